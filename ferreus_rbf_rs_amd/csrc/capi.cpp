// extern "C" boundary: include/ferreus_bbfmm_hip.h over bbfmm::FmmTree.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <memory>

#include "device_group.hpp"
#include "evaluate_grid.hpp"
#include "ferreus_bbfmm_hip.h"
#include "fmm_tree.hpp"
#include "interpolant_terms.hpp"
#include "field_program.hpp"
#include "closure_triangulate.hpp"
#include "isosurface.hpp"
#include "isosurface_closure.hpp"
#include "isosurface_curvature.hpp"
#include "isosurface_intersect.hpp"
#include "morton.hpp"

struct bbfmm_handle {
    bbfmm::FmmTree tree;                       // the handle's tree; part 0 of its device group when there is one
    std::unique_ptr<bbfmm::DeviceGroup> group; // several devices (or logical parts) behind this one handle
    std::string err;
    int64_t grid_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // of the last bbfmm_evaluate_grid (bbfmm_evaluate_grid_stats)
};

using bbfmm::FmmTree;

// A failure of the group: its message becomes the handle's.
static int group_rc(bbfmm_handle *h, int rc) {
    if (rc != BBFMM_OK) h->err = h->group->last_error();
    return rc;
}

namespace bbfmm {
void set_handle_error(bbfmm_handle *h, const char *message) { // interpolant.cpp: entry points outside this file
    if (h) h->err = message;
}
bool handle_is_host_only(const bbfmm_handle *h) { return h && h->tree.host_only(); } // solver_device.cpp, schwarz.cpp
} // namespace bbfmm

#define GUARD(h)                              \
    if (!(h)) return BBFMM_BAD_ARGUMENT;      \
    try {                                     \
        (h)->err.clear();                     \
        (h)->tree.bind_device();
#define END_GUARD(h)                                   \
    }                                                  \
    catch (const std::bad_alloc &) {                   \
        (h)->err = "out of host memory";               \
        return BBFMM_BAD_ARGUMENT;                     \
    }                                                  \
    catch (const std::exception &e) {                  \
        (h)->err = std::string("exception: ") + e.what(); \
        return BBFMM_BAD_ARGUMENT;                     \
    }                                                  \
    catch (...) {                                      \
        (h)->err = "unknown exception";                \
        return BBFMM_BAD_ARGUMENT;                     \
    }

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
        rc = h->group->evaluate_sharded(w, rows, k, ldw, x, m, ldx, out, ldo, nullptr, 0, false, false, bad_point_index, &handled);
        if (rc != BBFMM_OK || handled) return group_rc(h, rc);
        rc = group_rc(h, h->group->prepare_primary(h->group->weights_match_staged(w, rows, k, ldw)));
        if (rc != BBFMM_OK) return rc;
    }
    return h->tree.evaluate(w, rows, k, ldw, x, m, ldx, out, ldo, nullptr, 0, false, false, bad_point_index);
    END_GUARD(h)
}

int bbfmm_evaluate_with_gradients(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw,
                                  const double *x, int64_t m, int64_t ldx, double *out, int64_t ldo, double *grad,
                                  int64_t ldg, int64_t *bad_point_index) {
    GUARD(h)
    if (h->group) {
        bool handled = false;
        int rc = h->group->evaluate_sharded(w, rows, k, ldw, x, m, ldx, out, ldo, grad, ldg, true, false, bad_point_index, &handled);
        if (rc != BBFMM_OK || handled) return group_rc(h, rc);
        rc = group_rc(h, h->group->prepare_primary(!w || h->group->weights_match_staged(w, rows, k, ldw)));
        if (rc != BBFMM_OK) return rc;
    }
    return h->tree.evaluate(w, rows, k, ldw, x, m, ldx, out, ldo, grad, ldg, true, false, bad_point_index);
    END_GUARD(h)
}

int bbfmm_evaluate_leaves(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw, const double *x,
                          int64_t m, int64_t ldx, double *out, int64_t ldo, int64_t *bad_point_index) {
    GUARD(h)
    if (h->group) {
        bool handled = false;
        int rc = h->group->evaluate_sharded(w, rows, k, ldw, x, m, ldx, out, ldo, nullptr, 0, false, true, bad_point_index, &handled);
        if (rc != BBFMM_OK || handled) return group_rc(h, rc);
        rc = group_rc(h, h->group->prepare_primary(!w || h->group->weights_match_staged(w, rows, k, ldw)));
        if (rc != BBFMM_OK) return rc;
    }
    return h->tree.evaluate(w, rows, k, ldw, x, m, ldx, out, ldo, nullptr, 0, false, true, bad_point_index);
    END_GUARD(h)
}

int bbfmm_evaluate_leaves_with_gradients(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw,
                                         const double *x, int64_t m, int64_t ldx, double *out, int64_t ldo,
                                         double *grad, int64_t ldg, int64_t *bad_point_index) {
    GUARD(h)
    if (h->group) {
        bool handled = false;
        int rc = h->group->evaluate_sharded(w, rows, k, ldw, x, m, ldx, out, ldo, grad, ldg, true, true, bad_point_index, &handled);
        if (rc != BBFMM_OK || handled) return group_rc(h, rc);
        rc = group_rc(h, h->group->prepare_primary(!w || h->group->weights_match_staged(w, rows, k, ldw)));
        if (rc != BBFMM_OK) return rc;
    }
    return h->tree.evaluate(w, rows, k, ldw, x, m, ldx, out, ldo, grad, ldg, true, true, bad_point_index);
    END_GUARD(h)
}

// ---- isosurfaces (isosurface.hpp)
} // extern "C"

struct bbfmm_isosurface_result {
    std::vector<bbfmm::iso::Mesh> meshes;
    std::string err;
};

// Arguments shared by both extraction entry points; false with *err set on a bad one.
static bool iso_args(const double *extents, double resolution, const double *isovalues, int32_t n_iso,
                     bbfmm::iso::Lattice *lat, std::string *err) {
    if (!bbfmm::iso::make_lattice(extents, resolution, lat, err)) return false;
    if (n_iso < 1 || !isovalues) {
        *err = "isosurface: at least one isovalue is needed";
        return false;
    }
    for (int32_t q = 0; q < n_iso; ++q)
        if (!std::isfinite(isovalues[q])) {
            *err = "isosurface: isovalues must be finite";
            return false;
        }
    return true;
}

// The fields of *o that its size covers; defaults for the rest and for o == nullptr.
struct IsoFollow {
    int32_t follow = BBFMM_FOLLOW_DENSE;
    const double *seeds = nullptr;
    int64_t n_seeds = 0, seeds_ld = 0;
    const bbfmm_interpolant_terms *terms = nullptr;
};

// The field terms of one extraction on the device: the coefficients and the transformed copies of the targets of one
// field evaluation (grown on demand; every evaluation ends with its stream idle, so they are free to reuse).
struct IsoFieldTerms {
    bbfmm::InterpolantTerms t;
    bool on = false;
    double *d_lambda = nullptr, *xt[3] = {nullptr, nullptr, nullptr};
    int64_t cap = 0;
    ~IsoFieldTerms() {
        (void)hipFree(d_lambda);
        for (double *p : xt) (void)hipFree(p);
    }
    bool reserve(int64_t m) {
        if (m <= cap) return true;
        for (double *&p : xt) {
            (void)hipFree(p);
            p = nullptr;
        }
        cap = 0;
        for (double *&p : xt)
            if (hipMalloc(reinterpret_cast<void **>(&p), static_cast<size_t>(m) * sizeof(double)) != hipSuccess) return false;
        cap = m;
        return true;
    }
    // The checked copy of a caller's terms for a tree of dimension d (one column); false with *err set.
    bool init(const bbfmm_interpolant_terms *terms, int d, std::string *err) {
        const std::string dk = "d = " + std::to_string(d) + ", k = 1";
        if (!bbfmm::terms_from_abi(terms, &t) || t.d != d || t.k != 1) {
            *err = "bad field terms (" + dk + ", degree -1 .. 2, coefficients, scale != 0)";
            return false;
        }
        const int nb = bbfmm::terms_basis_size(d, t.degree);
        bool finite = true;
        for (int q = 0; q < nb; ++q) finite = finite && std::isfinite(t.lambda[q]);
        for (int q = 0; q < d * d && t.has_affine; ++q) finite = finite && std::isfinite(t.B[q]) && std::isfinite(t.b[q / d]);
        if (!finite) {
            *err = "field terms must be finite";
            return false;
        }
        on = nb > 0 || t.has_affine;
        return true;
    }
    // The polynomial coefficients on the tree's device (t.lambda is a device pointer from here on).
    bool upload(FmmTree &tree) {
        if (!on) return true;
        tree.bind_device();
        const int nb = bbfmm::terms_basis_size(t.d, t.degree);
        if (nb > 0) {
            if (hipMalloc(reinterpret_cast<void **>(&d_lambda), nb * sizeof(double)) != hipSuccess ||
                hipMemcpy(d_lambda, t.lambda, nb * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
                return false;
            t.lambda = d_lambda;
            t.ld_lambda = nb;
        }
        return true;
    }
    // The extents of the box [lo, hi] (t.d axes) as the tree sees it: of its 2^d transformed corners with a trend.
    void tree_box(double *lo, double *hi) const {
        if (!on || !t.has_affine) return;
        double l[3] = {0, 0, 0}, h[3] = {0, 0, 0};
        for (int c = 0; c < (1 << t.d); ++c) {
            double p[3] = {0, 0, 0}, q[3] = {0, 0, 0};
            for (int a = 0; a < t.d; ++a) p[a] = (c >> a) & 1 ? hi[a] : lo[a];
            bbfmm::affine_point(t, p, q);
            for (int a = 0; a < t.d; ++a) {
                l[a] = c == 0 ? q[a] : std::min(l[a], q[a]);
                h[a] = c == 0 ? q[a] : std::max(h[a], q[a]);
            }
        }
        for (int a = 0; a < t.d; ++a) {
            lo[a] = l[a];
            hi[a] = h[a];
        }
    }
    // The field of one interpolant at m device-resident points (x[a], a < t.d; the rest may be null): the tree is asked at
    // x B + b, the polynomial (and with grad the gradients: t.d columns of m) are added at x.  vals == nullptr: only the
    // tree's check that every point lies in it.  Without terms this is the tree's plain call.
    int eval(FmmTree &tree, const double *x0, const double *x1, const double *x2, int64_t m, double *vals, double *grad) {
        int64_t bad = -1;
        if (!on) return tree.evaluate_leaves_device(x0, x1, x2, m, vals, &bad, grad);
        const double *q[3] = {x0, x1, x2};
        if (t.has_affine && m > 0) {
            if (!reserve(m)) return BBFMM_DEVICE_ERROR;
            if (bbfmm::terms_affine_soa_device(t, x0, x1, x2, m, xt[0], xt[1], xt[2], tree.stream()) != 0) return BBFMM_DEVICE_ERROR;
            for (int a = 0; a < t.d; ++a) q[a] = xt[a];
        }
        // a deterministic handle gets the same double in every batching; a default one has f64 atomics between its M2P
        // jobs anyway and keeps the tuned plan
        const int rc = tree.evaluate_leaves_device(q[0], q[1], q[2], m, vals, &bad, grad, tree.deterministic());
        if (rc != BBFMM_OK || !vals) return rc;
        return bbfmm::terms_field_soa_device(t, x0, x1, x2, m, vals, grad, tree.stream()) == 0 ? BBFMM_OK : BBFMM_DEVICE_ERROR;
    }
};

static bool iso_options(const bbfmm_isosurface_options *o, int32_t *cluster, int32_t *finish, int64_t *batch_bytes,
                        int32_t *self_intersections, std::string *err, IsoFollow *fol = nullptr) {
    *cluster = BBFMM_CLUSTER_NONE;
    *finish = BBFMM_FINISH_RAW;
    *batch_bytes = 0;
    *self_intersections = BBFMM_SELF_INTERSECTIONS_IGNORE;
    if (!o) return true;
    if (o->size < static_cast<int64_t>(sizeof(int64_t))) {
        *err = "isosurface: options->size must be sizeof(bbfmm_isosurface_options)";
        return false;
    }
    if (o->size >= static_cast<int64_t>(offsetof(bbfmm_isosurface_options, cluster_method) + sizeof(int32_t))) *cluster = o->cluster_method;
    if (o->size >= static_cast<int64_t>(offsetof(bbfmm_isosurface_options, finish) + sizeof(int32_t))) *finish = o->finish;
    if (o->size >= static_cast<int64_t>(offsetof(bbfmm_isosurface_options, batch_bytes) + sizeof(int64_t))) *batch_bytes = o->batch_bytes;
    if (o->size >= static_cast<int64_t>(offsetof(bbfmm_isosurface_options, self_intersections) + sizeof(int32_t)))
        *self_intersections = o->self_intersections;
    // follow lies in what was padding after self_intersections, which an older caller's size covers without having set
    // it: it is read together with the seeds, from a struct that holds them all
    if (fol && o->size >= static_cast<int64_t>(offsetof(bbfmm_isosurface_options, seeds_ld) + sizeof(int64_t))) {
        fol->follow = o->follow;
        fol->seeds = o->seeds;
        fol->n_seeds = o->n_seeds;
        fol->seeds_ld = o->seeds_ld;
    }
    if (fol && o->size >= static_cast<int64_t>(offsetof(bbfmm_isosurface_options, terms) + sizeof(void *))) fol->terms = o->terms;
    return true;
}

static bool iso_follow_ok(const IsoFollow &fol, bool need_seeds, std::string *err) {
    if (fol.follow != BBFMM_FOLLOW_DENSE && fol.follow != BBFMM_FOLLOW_SURFACE) {
        *err = "isosurface: unknown follow mode " + std::to_string(fol.follow);
        return false;
    }
    if (fol.follow == BBFMM_FOLLOW_DENSE) return true;
    if (fol.n_seeds < 0 || (fol.n_seeds > 0 && (!fol.seeds || fol.seeds_ld < fol.n_seeds))) {
        *err = "isosurface: seeds must hold n_seeds >= 0 points with seeds_ld >= n_seeds";
        return false;
    }
    if (need_seeds && !fol.seeds && fol.n_seeds == 0) {
        // (an empty array of seeds is given as a non-null pointer with n_seeds = 0)
        *err = "isosurface: follow=surface of a caller's values needs seeds";
        return false;
    }
    return true;
}

static bool iso_methods_ok(int32_t cluster, int32_t finish, int32_t self_intersections, std::string *err) {
    if (self_intersections != BBFMM_SELF_INTERSECTIONS_IGNORE && self_intersections != BBFMM_SELF_INTERSECTIONS_ROLLBACK) {
        *err = "isosurface: unknown self-intersection handling " + std::to_string(self_intersections);
        return false;
    }
    if (cluster != BBFMM_CLUSTER_NONE && cluster != BBFMM_CLUSTER_AVERAGE && cluster != BBFMM_CLUSTER_CURVATURE) {
        *err = "isosurface: unknown cluster method " + std::to_string(cluster);
        return false;
    }
    if (finish < BBFMM_FINISH_RAW || finish > BBFMM_FINISH_CLOSE_NEGATIVE) {
        *err = "isosurface: unknown finish " + std::to_string(finish);
        return false;
    }
    return true;
}

// BBFMM_ISO_SEED_GRADIENTS (read per call): `differences` takes the reference's central differences of the values
// (seed_projection.rs:138-189), which a kernel without gradients takes anyway; `leaf_pass`, empty or unset: the field's own
// gradients (*own).  false with *err set for anything else.
static bool iso_seed_gradients(bool *own, std::string *err) {
    const char *sg = std::getenv("BBFMM_ISO_SEED_GRADIENTS");
    if (sg && *sg && std::strcmp(sg, "differences") != 0 && std::strcmp(sg, "leaf_pass") != 0) {
        *err = std::string("isosurface: BBFMM_ISO_SEED_GRADIENTS must be leaf_pass or differences, got '") + sg + "'";
        return false;
    }
    *own = !(sg && !std::strcmp(sg, "differences"));
    return true;
}

static int iso_fail(bbfmm_handle *h, bbfmm_isosurface_result *r, int rc, const std::string &msg) {
    if (h) h->err = msg;
    if (r) r->err = msg;
    return rc;
}

extern "C" {

int bbfmm_isosurface_tables(int32_t *edge_deltas, int32_t *reverse_edge, int32_t *owned_tet_edges,
                            int32_t *tet_edge_pairs, int32_t *mt_table) {
    using namespace bbfmm::iso;
    if (!edge_deltas || !reverse_edge || !owned_tet_edges || !tet_edge_pairs || !mt_table) return BBFMM_BAD_ARGUMENT;
    for (int e = 0; e < 14; ++e) {
        for (int a = 0; a < 3; ++a) edge_deltas[3 * e + a] = kEdgeDeltas[e][a];
        reverse_edge[e] = kReverseEdge[e];
    }
    for (int t = 0; t < 6; ++t) {
        for (int a = 0; a < 3; ++a) owned_tet_edges[3 * t + a] = kOwnedTetEdges[t][a];
        for (int a = 0; a < 2; ++a) tet_edge_pairs[2 * t + a] = kTetEdgePairs[t][a];
    }
    for (int c = 0; c < 16; ++c) {
        mt_table[7 * c] = kMtCount[c];
        for (int r = 0; r < 2; ++r)
            for (int a = 0; a < 3; ++a) mt_table[7 * c + 1 + 3 * r + a] = r < kMtCount[c] ? kMtTable[c][r][a] : -1;
    }
    return BBFMM_OK;
}

int bbfmm_isosurface_lattice(bbfmm_handle *h, const double *extents, double resolution, int64_t *info_out) {
    if (!info_out) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, "isosurface: info_out must not be null");
    bbfmm::iso::Lattice lat;
    std::string err;
    try {
        if (!bbfmm::iso::make_lattice(extents, resolution, &lat, &err)) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, err);
    } catch (const std::bad_alloc &) {
        return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, "out of host memory");
    }
    for (int a = 0; a < 3; ++a) {
        info_out[a] = lat.max_ijk[a];
        info_out[5 + a] = lat.lo[a];
        info_out[8 + a] = lat.dims[a];
    }
    info_out[3] = lat.n_keys;
    info_out[4] = lat.n_nodes;
    if (h) h->err.clear();
    return BBFMM_OK;
}

int bbfmm_isosurface_cluster_tables(int32_t *neighbour_masks, int32_t *flat_hole_masks, int32_t *all14_mask) {
    using namespace bbfmm::iso;
    if (!neighbour_masks || !flat_hole_masks || !all14_mask) return BBFMM_BAD_ARGUMENT;
    for (int e = 0; e < 14; ++e) neighbour_masks[e] = kNeighbourMasks[e];
    for (int r = 0; r < 36; ++r)
        for (int a = 0; a < 2; ++a) flat_hole_masks[2 * r + a] = kFlatHoleMasks[r][a];
    *all14_mask = kAll14;
    return BBFMM_OK;
}

int bbfmm_isosurface_curvature_tables(int32_t *plane_pairs, int32_t *plane_phis, double *constants) {
    using namespace bbfmm::iso;
    if (!plane_pairs || !plane_phis || !constants) return BBFMM_BAD_ARGUMENT;
    for (int l = 0; l < 7; ++l)
        for (int p = 0; p < 3; ++p)
            for (int side = 0; side < 2; ++side) {
                const bool used = p < kCurvPlanes[l];
                plane_pairs[(l * 3 + p) * 2 + side] = used ? kCurvPairs[l][p][side] : -1;
                plane_phis[(l * 3 + p) * 2 + side] = used ? kCurvPhis[l][p][side] + 1 : -1;
            }
    constants[0] = kCurvPhi[0];
    constants[1] = kCurvPhi[1];
    constants[2] = kCurvEps;
    constants[3] = kCurvMaxCot;
    constants[4] = kCurvMaxWeight;
    return BBFMM_OK;
}

int bbfmm_isosurface_curvature_weight(const double *values, const int64_t *owner_ijk, int32_t label, const double *lo_world,
                                      const double *spacing, double *weight_out, int32_t *fallback_out) {
    using namespace bbfmm::iso;
    if (!values || !owner_ijk || !lo_world || !spacing || !weight_out || label < 0 || label >= 7) return BBFMM_BAD_ARGUMENT;
    const auto get = [values](int e) { return values[e + 1]; };
    double w = 1.0;
    const bool ok = curvature_weight(get, owner_ijk, label, lo_world, spacing, curvature_trig(), &w);
    *weight_out = ok ? w : 1.0;
    if (fallback_out) *fallback_out = ok ? 0 : 1;
    return BBFMM_OK;
}

int bbfmm_isosurface_topology(uint32_t near_mask, const double *neighbour_values, int32_t *case_out, int32_t *cluster_of_edge) {
    using namespace bbfmm::iso;
    if (!case_out || !cluster_of_edge || near_mask > kAll14) return BBFMM_BAD_ARGUMENT;
    int c = kSimple;
    const uint64_t part = topology_partition(static_cast<uint16_t>(near_mask), neighbour_values, &c);
    *case_out = c;
    for (int e = 0; e < 14; ++e) cluster_of_edge[e] = part_label(part, e) == 15 ? -1 : part_label(part, e);
    return BBFMM_OK;
}

int bbfmm_build_isosurfaces(bbfmm_handle *h, const double *extents, double resolution, const double *isovalues,
                            int32_t n_isovalues, const double *drift, double *d_field_out, int64_t batch_bytes,
                            bbfmm_isosurface_result **out) {
    return bbfmm_build_isosurfaces_ex(h, extents, resolution, isovalues, n_isovalues, drift, d_field_out, batch_bytes,
                                      BBFMM_CLUSTER_NONE, out);
}

} // extern "C"

static int build_isosurfaces_impl(bbfmm_handle *h, const double *extents, double resolution, const double *isovalues,
                                  int32_t n_isovalues, const double *drift, double *d_field_out, int64_t batch_bytes,
                                  int32_t cluster_method, int32_t finish, int32_t self_intersections,
                                  bbfmm_isosurface_result **out, const IsoFollow &fol = IsoFollow()) {
    GUARD(h)
    if (out) *out = nullptr;
    if (!out) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, "isosurface: out must not be null");
    {
        std::string bad;
        if (!iso_methods_ok(cluster_method, finish, self_intersections, &bad)) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, bad);
        if (!iso_follow_ok(fol, false, &bad)) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, bad);
    }
    if (h->tree.tree().d != 3) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, "isosurface: only supported for 3D (d = 3)");
    bbfmm::iso::Lattice lat;
    std::string err;
    if (!iso_args(extents, resolution, isovalues, n_isovalues, &lat, &err)) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, err);
    if (drift)
        for (int a = 0; a < 4; ++a)
            if (!std::isfinite(drift[a])) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, "isosurface: drift must be finite");
    if (h->tree.host_only()) return iso_fail(h, nullptr, BBFMM_DEVICE_ERROR, "handle was created with BBFMM_FLAG_HOST_ONLY");
    if (h->group) {
        const int rc = group_rc(h, h->group->prepare_primary(true)); // the stored expansions of the primary (Leaves mode)
        if (rc != BBFMM_OK) return rc;
    }
    FmmTree &t = h->tree;
    IsoFieldTerms ft;
    if (fol.terms) {
        if (drift) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, "isosurface: give the drift or the field terms, not both");
        std::string bad;
        if (!ft.init(fol.terms, 3, &bad)) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, "isosurface: " + bad);
        if (ft.t.has_affine && fol.follow == BBFMM_FOLLOW_SURFACE && !fol.seeds)
            return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, "isosurface: with a global trend the seeds must be given (world points)");
    }
    // every node of E inside the tree's cube (points_to_leaves saturates coordinates below the tree, as the reference's
    // Morton encoding does, so the bounds are checked here); the device pass of extract() then finds every leaf.
    // With a global trend: the extents of the 8 transformed corners of the lattice box (rbf.rs:599-613).
    double box_lo[3], box_hi[3];
    for (int a = 0; a < 3; ++a) {
        box_lo[a] = lat.lo_world[a] + static_cast<double>(lat.lo[a]) * lat.spacing[a];
        box_hi[a] = lat.lo_world[a] + static_cast<double>(lat.lo[a] + lat.dims[a] - 1) * lat.spacing[a];
    }
    ft.tree_box(box_lo, box_hi);
    for (int a = 0; a < 3; ++a) {
        const auto &tr = t.tree();
        const double w0 = box_lo[a], w1 = box_hi[a];
        if (!(w0 >= tr.center[a] - tr.radius) || !(w1 <= tr.center[a] + tr.radius))
            return iso_fail(h, nullptr, BBFMM_POINT_OUTSIDE_TREE,
                            "isosurface: lattice nodes on axis " + std::to_string(a) + " span [" + std::to_string(w0) + ", " +
                                std::to_string(w1) + "], outside the tree extents [" + std::to_string(tr.center[a] - tr.radius) +
                                ", " + std::to_string(tr.center[a] + tr.radius) + "] (pad the tree's extents, as rbf.rs:992-998 does)");
    }
    bbfmm::iso::FieldFn fn = [&t](const double *x0, const double *x1, const double *x2, int64_t m, double *vals) {
        int64_t bad = -1;
        return t.evaluate_leaves_device(x0, x1, x2, m, vals, &bad);
    };
    // with field terms: the tree is asked at x B + b, the polynomial (and for the seeds the gradients) are added at x
    // (IsoFieldTerms::eval, shared with the operands of a composite field)
    auto with_terms = [&t, &ft](const double *x0, const double *x1, const double *x2, int64_t m, double *vals, double *grad) -> int {
        return ft.eval(t, x0, x1, x2, m, vals, grad);
    };
    if (ft.on) {
        if (!ft.upload(t)) return iso_fail(h, nullptr, BBFMM_DEVICE_ERROR, "isosurface: upload of the field terms");
        fn = [&with_terms](const double *x0, const double *x1, const double *x2, int64_t m, double *vals) {
            return with_terms(x0, x1, x2, m, vals, nullptr);
        };
    }
    bbfmm::iso::Request req;
    req.isovalues = isovalues;
    req.n_iso = n_isovalues;
    req.drift = drift;
    req.d_field_out = d_field_out;
    req.budget_bytes = batch_bytes;
    req.cluster = cluster_method;
    req.finish = finish;
    req.extents = extents;
    req.self_intersections = self_intersections;
    req.follow = fol.follow;
    if (fol.follow == BBFMM_FOLLOW_SURFACE) {
        if (fol.seeds) {
            req.seeds = fol.seeds;
            req.n_seeds = fol.n_seeds;
            req.seeds_ld = fol.seeds_ld;
        } else { // the data points (rbf.rs:1049)
            req.seeds = t.source_points().data();
            req.n_seeds = req.seeds_ld = t.tree().n_points;
        }
        bool own_gradients = false;
        if (!iso_seed_gradients(&own_gradients, &err)) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, err);
        if (t.supports_gradients() && own_gradients)
            req.grad = [&t](const double *x0, const double *x1, const double *x2, int64_t m, double *vals, double *grad) {
                int64_t bad = -1;
                return t.evaluate_leaves_device(x0, x1, x2, m, vals, &bad, grad);
            };
        if (req.grad && ft.on) req.grad = with_terms;
    }
    std::unique_ptr<bbfmm_isosurface_result> r(new bbfmm_isosurface_result());
    const int rc = bbfmm::iso::extract(lat, fn, req, t.stream(), &r->meshes, &err);
    if (rc != BBFMM_OK) {
        // a failure of the field evaluation has its message in the tree
        if (err.empty()) err = t.last_error();
        return iso_fail(h, nullptr, rc, err);
    }
    *out = r.release();
    return BBFMM_OK;
    END_GUARD(h)
}

// A host mesh (mesh_op: clip and clean, or the self-intersection detector) or a host field through extract(), on the
// handle's stream or one of the call's own.
enum IsoMeshOp : int { kIsoField = 0, kIsoFinishMesh = 1, kIsoDetectMesh = 2, kIsoCloseMesh = 3 };
static int isosurfaces_from_host(bbfmm_handle *h, const double *values, const double *extents, double resolution,
                                 const double *isovalues, int32_t n_isovalues, int64_t batch_bytes, int32_t cluster_method,
                                 int32_t finish, int32_t self_intersections, const double *vertices, int64_t n_vertices,
                                 const int64_t *facets, int64_t n_facets, int mesh_op, bbfmm_isosurface_result **out,
                                 const IsoFollow &fol = IsoFollow()) {
    const bool one_mesh = mesh_op != kIsoField, detect = mesh_op == kIsoDetectMesh;
    if (!out) return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, "isosurface: out must not be null");
    *out = nullptr;
    bbfmm_isosurface_result *r = nullptr;
    try {
        r = new bbfmm_isosurface_result();
        *out = r;
        if (h) {
            h->err.clear();
            h->tree.bind_device();
        }
        bbfmm::iso::Lattice lat;
        bbfmm::iso::ClipBox box;
        std::string err;
        if (one_mesh) {
            // everything is checked before any work: the box, the sizes the id packing holds, the ids
            if ((!detect || extents) && !bbfmm::iso::make_clip_box(extents, &box, &err)) return iso_fail(h, r, BBFMM_BAD_ARGUMENT, err);
            if (!detect && !bbfmm::iso::finish_fits(n_vertices, n_facets, &err)) return iso_fail(h, r, BBFMM_BAD_ARGUMENT, err);
            if ((n_vertices > 0 && !vertices) || (n_facets > 0 && !facets))
                return iso_fail(h, r, BBFMM_BAD_ARGUMENT, "isosurface: vertices and facets must not be null");
            for (int64_t q = 0; q < 3 * n_facets; ++q)
                if (facets[q] < 0 || facets[q] >= n_vertices)
                    return iso_fail(h, r, BBFMM_BAD_ARGUMENT, "isosurface: facet " + std::to_string(q / 3) + " names vertex " +
                                                                  std::to_string(facets[q]) + " of " + std::to_string(n_vertices));
            if (detect)
                for (int64_t q = 0; q < 3 * n_vertices; ++q)
                    if (!std::isfinite(vertices[q]))
                        return iso_fail(h, r, BBFMM_BAD_ARGUMENT, "isosurface: vertex " + std::to_string(q / 3) + " is not finite");
        } else {
            if (!iso_args(extents, resolution, isovalues, n_isovalues, &lat, &err)) return iso_fail(h, r, BBFMM_BAD_ARGUMENT, err);
            if (!values) return iso_fail(h, r, BBFMM_BAD_ARGUMENT, "isosurface: values must not be null");
            if (!iso_methods_ok(cluster_method, finish, self_intersections, &err)) return iso_fail(h, r, BBFMM_BAD_ARGUMENT, err);
            if (!iso_follow_ok(fol, true, &err)) return iso_fail(h, r, BBFMM_BAD_ARGUMENT, err);
        }
        if (h && h->tree.host_only()) return iso_fail(h, r, BBFMM_DEVICE_ERROR, "handle was created with BBFMM_FLAG_HOST_ONLY");
        if (h && h->group) {
            const int rc = group_rc(h, h->group->prepare_primary(true));
            if (rc != BBFMM_OK) return iso_fail(h, r, rc, h->err);
        }
        hipStream_t st = h ? h->tree.stream() : nullptr;
        bool own = false;
        if (!h) {
            const hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
            if (e != hipSuccess) return iso_fail(h, r, BBFMM_DEVICE_ERROR, std::string("isosurface: hipStreamCreate: ") + hipGetErrorString(e));
            own = true;
        }
        int rc = BBFMM_OK;
        if (one_mesh) {
            r->meshes.assign(1, bbfmm::iso::Mesh());
            double *d_v = nullptr;
            int64_t *d_f = nullptr;
            uint8_t *d_flag = nullptr;
            hipError_t e = hipSuccess;
            if (n_facets > 0) {
                e = hipMalloc(reinterpret_cast<void **>(&d_v), 3 * static_cast<size_t>(n_vertices) * sizeof(double));
                if (e == hipSuccess && detect) e = hipMalloc(reinterpret_cast<void **>(&d_flag), static_cast<size_t>(n_facets));
                if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_f), 3 * static_cast<size_t>(n_facets) * sizeof(int64_t));
                if (e == hipSuccess) e = hipMemcpyAsync(d_v, vertices, 3 * static_cast<size_t>(n_vertices) * sizeof(double), hipMemcpyHostToDevice, st);
                if (e == hipSuccess) e = hipMemcpyAsync(d_f, facets, 3 * static_cast<size_t>(n_facets) * sizeof(int64_t), hipMemcpyHostToDevice, st);
                if (e == hipSuccess) e = hipStreamSynchronize(st); // (pageable sources)
            }
            if (e != hipSuccess) {
                rc = BBFMM_DEVICE_ERROR;
                err = std::string("isosurface: upload of the mesh: ") + hipGetErrorString(e);
            } else if (detect) {
                bbfmm::iso::Mesh &m = r->meshes[0];
                rc = bbfmm::iso::self_intersections_device(d_v, n_vertices, d_f, n_facets, extents ? &box : nullptr, st, d_flag,
                                                           m.isect_stats, &err);
                if (rc == BBFMM_OK && m.isect_stats[bbfmm::iso::kIsectTriangles] > 0) { // the sorted ids: the flags in facet order
                    std::vector<uint8_t> flag(static_cast<size_t>(n_facets));
                    e = hipMemcpyAsync(flag.data(), d_flag, flag.size(), hipMemcpyDeviceToHost, st);
                    if (e == hipSuccess) e = hipStreamSynchronize(st);
                    if (e != hipSuccess) {
                        rc = BBFMM_DEVICE_ERROR;
                        err = std::string("isosurface: download of the flags: ") + hipGetErrorString(e);
                    }
                    for (int64_t t = 0; rc == BBFMM_OK && t < n_facets; ++t)
                        if (flag[t]) m.isect_ids.push_back(t);
                }
            } else if (mesh_op == kIsoCloseMesh) { // the closure alone (finish: the mode)
                rc = bbfmm::iso::closure_device(d_v, n_vertices, d_f, n_facets, box, resolution, finish, st, &r->meshes[0], &err);
                if (rc == BBFMM_OK && n_facets == 0 && n_vertices > 0) r->meshes[0].vertices.assign(vertices, vertices + 3 * n_vertices);
            } else {
                rc = bbfmm::iso::finish_device(d_v, n_vertices, d_f, n_facets, box, st, &r->meshes[0], &err);
            }
            (void)hipFree(d_v);
            (void)hipFree(d_f);
            (void)hipFree(d_flag);
        } else {
            bbfmm::iso::Request req;
            req.isovalues = isovalues;
            req.n_iso = n_isovalues;
            req.host_field = values;
            req.budget_bytes = batch_bytes;
            req.cluster = cluster_method;
            req.finish = finish;
            req.extents = extents;
            req.self_intersections = self_intersections;
            req.follow = fol.follow;
            req.seeds = fol.seeds;
            req.n_seeds = fol.n_seeds;
            req.seeds_ld = fol.seeds_ld;
            rc = bbfmm::iso::extract(lat, bbfmm::iso::FieldFn(), req, st, &r->meshes, &err);
        }
        if (own) (void)hipStreamDestroy(st);
        if (rc != BBFMM_OK) return iso_fail(h, r, rc, err);
        return BBFMM_OK;
    } catch (const std::bad_alloc &) {
        return iso_fail(h, r, BBFMM_BAD_ARGUMENT, "out of host memory");
    } catch (const std::exception &e) {
        return iso_fail(h, r, BBFMM_BAD_ARGUMENT, std::string("exception: ") + e.what());
    }
}

// ---- composite fields and callers' functions (field_program.hpp; DESIGN.md "Composite fields")
namespace {

struct DevColumn { // grows only, freed with the call
    double *p = nullptr;
    int64_t cap = 0;
    DevColumn() = default;
    DevColumn(const DevColumn &) = delete;
    DevColumn &operator=(const DevColumn &) = delete;
    ~DevColumn() { (void)hipFree(p); }
    bool reserve(int64_t n) {
        if (n <= cap) return true;
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(reinterpret_cast<void **>(&p), static_cast<size_t>(n) * sizeof(double)) != hipSuccess) return false;
        cap = n;
        return true;
    }
};

struct FieldOperand {
    int kind = BBFMM_FIELD_AFFINE, axis = 2;
    bbfmm_handle *h = nullptr;
    IsoFieldTerms ft;
    double affine[4] = {0, 0, 0, 0};
    DevColumn v, g; // the operand's values and, for the seed projection, its 3 gradient columns
    int d() const { return kind == BBFMM_FIELD_MODEL ? 3 : 2; }
    // the axes of the lattice the operand's tree sees, in its own order
    void axes(int *out) const {
        if (kind == BBFMM_FIELD_MODEL) {
            out[0] = 0, out[1] = 1, out[2] = 2;
        } else {
            out[0] = axis == 0 ? 1 : 0, out[1] = axis == 2 ? 1 : 2, out[2] = -1;
        }
    }
};

struct CompositeField {
    std::unique_ptr<FieldOperand[]> ops;
    int n = 0;
    bbfmm::FieldProgram prog;
    hipStream_t st = nullptr; // the extraction's stream
    std::string err;

    // Everything about the operands and the program that the host can check; false with *msg set.
    bool setup(const bbfmm_field_operand *operands, int32_t n_operands, const int32_t *program, int32_t n_program, std::string *msg) {
        if (n_operands < 1 || n_operands > bbfmm::kFieldMaxOperands || !operands) {
            *msg = "isosurface: " + std::to_string(n_operands) + " operands (1 .. " + std::to_string(bbfmm::kFieldMaxOperands) + ")";
            return false;
        }
        ops.reset(new FieldOperand[n_operands]);
        n = n_operands;
        double scale[bbfmm::kFieldMaxOperands], offset[bbfmm::kFieldMaxOperands];
        int device = -1;
        for (int o = 0; o < n; ++o) {
            const bbfmm_field_operand &in = operands[o];
            FieldOperand &op = ops[o];
            const std::string at = "isosurface: operand " + std::to_string(o) + ": ";
            if (in.size < static_cast<int64_t>(sizeof(bbfmm_field_operand))) {
                *msg = at + "size must be sizeof(bbfmm_field_operand)";
                return false;
            }
            if (in.kind != BBFMM_FIELD_MODEL && in.kind != BBFMM_FIELD_HEIGHT && in.kind != BBFMM_FIELD_AFFINE) {
                *msg = at + "unknown kind " + std::to_string(in.kind);
                return false;
            }
            op.kind = in.kind;
            scale[o] = in.scale;
            offset[o] = in.offset;
            if (!std::isfinite(in.scale) || !std::isfinite(in.offset)) {
                *msg = at + "scale and offset must be finite";
                return false;
            }
            if (in.kind == BBFMM_FIELD_AFFINE) {
                for (int a = 0; a < 4; ++a) {
                    if (!std::isfinite(in.affine[a])) {
                        *msg = at + "affine coefficients must be finite";
                        return false;
                    }
                    op.affine[a] = in.affine[a];
                }
                if (in.handle || in.terms) {
                    *msg = at + "an affine operand takes no handle and no terms";
                    return false;
                }
                continue;
            }
            if (!in.handle) {
                *msg = at + "a handle is needed";
                return false;
            }
            op.h = in.handle;
            bbfmm::FmmTree &t = op.h->tree;
            if (in.kind == BBFMM_FIELD_HEIGHT) {
                if (in.axis < 0 || in.axis > 2) {
                    *msg = at + "axis must be 0, 1 or 2, got " + std::to_string(in.axis);
                    return false;
                }
                op.axis = in.axis;
            }
            if (t.tree().d != op.d()) {
                *msg = at + (in.kind == BBFMM_FIELD_MODEL ? "a model operand needs a handle with d = 3" : "a height operand needs a handle with d = 2") +
                       ", got d = " + std::to_string(t.tree().d);
                return false;
            }
            if (t.host_only()) {
                *msg = at + "handle was created with BBFMM_FLAG_HOST_ONLY";
                return false;
            }
            if (op.h->group) {
                *msg = at + "a handle on a device group cannot be an operand";
                return false;
            }
            if (!t.leaves_ready()) {
                *msg = at + "set_local_coefficients (one column) must be called first";
                return false;
            }
            if (device < 0) device = t.device();
            if (t.device() != device) {
                *msg = at + "its handle is on device " + std::to_string(t.device()) + ", the first one on device " + std::to_string(device);
                return false;
            }
            if (in.terms) {
                std::string bad;
                if (!op.ft.init(in.terms, op.d(), &bad)) {
                    *msg = at + bad;
                    return false;
                }
            }
        }
        std::string bad;
        if (!bbfmm::field_program_make(n, scale, offset, program, n_program, &prog, &bad)) {
            *msg = "isosurface: " + bad;
            return false;
        }
        return true;
    }

    // The lattice box [lo, hi] inside every tree operand's cube (square); BBFMM_POINT_OUTSIDE_TREE with *msg otherwise.
    int inside(const double *box_lo, const double *box_hi, std::string *msg) const {
        for (int o = 0; o < n; ++o) {
            const FieldOperand &op = ops[o];
            if (!op.h) continue;
            int ax[3];
            op.axes(ax);
            double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
            for (int a = 0; a < op.d(); ++a) {
                lo[a] = box_lo[ax[a]];
                hi[a] = box_hi[ax[a]];
            }
            op.ft.tree_box(lo, hi);
            const auto &tr = op.h->tree.tree();
            for (int a = 0; a < op.d(); ++a)
                if (!(lo[a] >= tr.center[a] - tr.radius) || !(hi[a] <= tr.center[a] + tr.radius)) {
                    *msg = "isosurface: operand " + std::to_string(o) + ": lattice nodes on its axis " + std::to_string(a) + " span [" +
                           std::to_string(lo[a]) + ", " + std::to_string(hi[a]) + "], outside the tree extents [" +
                           std::to_string(tr.center[a] - tr.radius) + ", " + std::to_string(tr.center[a] + tr.radius) +
                           "] (pad the tree's extents, as rbf.rs:992-998 does)";
                    return BBFMM_POINT_OUTSIDE_TREE;
                }
        }
        return BBFMM_OK;
    }

    bool gradients() const {
        for (int o = 0; o < n; ++o)
            if (ops[o].h && !ops[o].h->tree.supports_gradients()) return false;
        return true;
    }

    // FieldFn / GradFn: one column per operand, then the program.  vals == nullptr: every tree's own check of the points.
    int eval(const double *x0, const double *x1, const double *x2, int64_t m, double *vals, double *grad) {
        if (m <= 0) return BBFMM_OK;
        if (hipStreamSynchronize(st) != hipSuccess) { // the coordinates are there; the columns of the last call are free
            err = "isosurface: hipStreamSynchronize before the operands";
            return BBFMM_DEVICE_ERROR;
        }
        const double *x[3] = {x0, x1, x2};
        bbfmm::FieldColumns c;
        for (int o = 0; o < n; ++o) {
            FieldOperand &op = ops[o];
            const std::string at = "isosurface: operand " + std::to_string(o) + ": ";
            if (vals && (!op.v.reserve(m) || (grad && !op.g.reserve(3 * m)))) {
                err = at + "out of device memory for its column";
                return BBFMM_DEVICE_ERROR;
            }
            double *gv = grad ? op.g.p : nullptr;
            if (!op.h) {
                if (vals && bbfmm::field_affine_device(op.affine, x0, x1, x2, m, op.v.p, gv, st) != 0) {
                    err = at + "the affine kernel";
                    return BBFMM_DEVICE_ERROR;
                }
            } else {
                bbfmm::FmmTree &t = op.h->tree;
                int ax[3];
                op.axes(ax);
                const int rc = op.ft.eval(t, x[ax[0]], x[ax[1]], ax[2] < 0 ? nullptr : x[ax[2]], m, vals ? op.v.p : nullptr, gv);
                if (rc != BBFMM_OK) {
                    err = at + t.last_error();
                    return rc;
                }
                if (vals) {
                    // (the terms kernel is queued on the tree's stream and not synchronised)
                    if (op.ft.on && t.stream() != st && hipStreamSynchronize(t.stream()) != hipSuccess) {
                        err = at + "hipStreamSynchronize after its terms";
                        return BBFMM_DEVICE_ERROR;
                    }
                    if (op.kind == BBFMM_FIELD_HEIGHT && bbfmm::field_height_device(op.axis, x[op.axis], m, op.v.p, gv, st) != 0) {
                        err = at + "the height kernel";
                        return BBFMM_DEVICE_ERROR;
                    }
                }
            }
            c.v[o] = op.v.p;
            c.g[o] = gv;
            c.ldg[o] = m;
        }
        if (!vals) return BBFMM_OK;
        if (bbfmm::field_program_device(prog, c, m, vals, grad, st) != 0) {
            err = "isosurface: the field program kernel";
            return BBFMM_DEVICE_ERROR;
        }
        return BBFMM_OK;
    }
};

// A caller's host function as the field: every batch is downloaded, handed over and its values uploaded.
struct FunctionField {
    bbfmm_field_fn field = nullptr;
    bbfmm_gradient_fn gradient = nullptr;
    void *user = nullptr;
    hipStream_t st = nullptr;
    std::vector<double> x, v, g;
    std::string err;

    int eval(const double *x0, const double *x1, const double *x2, int64_t m, double *vals, double *grad) {
        if (m <= 0 || !vals) return BBFMM_OK;
        const size_t sm = static_cast<size_t>(m), bytes = sm * sizeof(double);
        x.resize(3 * sm);
        v.resize(sm);
        if (grad) g.resize(3 * sm);
        const double *xs[3] = {x0, x1, x2};
        hipError_t e = hipSuccess;
        for (int a = 0; a < 3 && e == hipSuccess; ++a) e = hipMemcpyAsync(x.data() + a * sm, xs[a], bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            err = std::string("isosurface: download of the nodes: ") + hipGetErrorString(e);
            return BBFMM_DEVICE_ERROR;
        }
        const int rc = grad ? gradient(x.data(), m, m, v.data(), g.data(), m, user) : field(x.data(), m, m, v.data(), user);
        if (rc != 0) {
            err = "isosurface: the field callback returned " + std::to_string(rc);
            return BBFMM_CALLBACK_FAILED;
        }
        e = hipMemcpyAsync(vals, v.data(), bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && grad) e = hipMemcpyAsync(grad, g.data(), 3 * bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st); // (pageable sources, reused by the next call)
        if (e != hipSuccess) {
            err = std::string("isosurface: upload of the values: ") + hipGetErrorString(e);
            return BBFMM_DEVICE_ERROR;
        }
        return BBFMM_OK;
    }
};

struct OwnStream {
    hipStream_t st = nullptr;
    ~OwnStream() {
        if (st) (void)hipStreamDestroy(st);
    }
};

// What both entries share: options, lattice, request.  seed_gradients: 1 when the seed projection may take a GradFn.
int field_request(const double *extents, double resolution, const double *isovalues, int32_t n_isovalues, double *d_field_out,
                  const bbfmm_isosurface_options *options, bbfmm::iso::Lattice *lat, bbfmm::iso::Request *req, bool *seed_gradients,
                  std::string *err) {
    int32_t cluster, finish, isect;
    int64_t batch;
    IsoFollow fol;
    if (!iso_options(options, &cluster, &finish, &batch, &isect, err, &fol)) return BBFMM_BAD_ARGUMENT;
    if (fol.terms) {
        *err = "isosurface: options->terms must be NULL here (terms belong to operands)";
        return BBFMM_BAD_ARGUMENT;
    }
    if (!iso_methods_ok(cluster, finish, isect, err) || !iso_follow_ok(fol, true, err)) return BBFMM_BAD_ARGUMENT;
    if (!iso_args(extents, resolution, isovalues, n_isovalues, lat, err)) return BBFMM_BAD_ARGUMENT;
    req->isovalues = isovalues;
    req->n_iso = n_isovalues;
    req->d_field_out = d_field_out;
    req->budget_bytes = batch;
    req->cluster = cluster;
    req->finish = finish;
    req->extents = extents;
    req->self_intersections = isect;
    req->follow = fol.follow;
    *seed_gradients = false;
    if (fol.follow == BBFMM_FOLLOW_SURFACE) {
        req->seeds = fol.seeds;
        req->n_seeds = fol.n_seeds;
        req->seeds_ld = fol.seeds_ld;
        if (!iso_seed_gradients(seed_gradients, err)) return BBFMM_BAD_ARGUMENT;
    }
    return BBFMM_OK;
}

} // namespace

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

int bbfmm_build_isosurfaces_ex(bbfmm_handle *h, const double *extents, double resolution, const double *isovalues,
                               int32_t n_isovalues, const double *drift, double *d_field_out, int64_t batch_bytes,
                               int32_t cluster_method, bbfmm_isosurface_result **out) {
    return build_isosurfaces_impl(h, extents, resolution, isovalues, n_isovalues, drift, d_field_out, batch_bytes, cluster_method,
                                  BBFMM_FINISH_RAW, BBFMM_SELF_INTERSECTIONS_IGNORE, out);
}

int bbfmm_build_isosurfaces_opts(bbfmm_handle *h, const double *extents, double resolution, const double *isovalues,
                                 int32_t n_isovalues, const double *drift, double *d_field_out,
                                 const bbfmm_isosurface_options *options, bbfmm_isosurface_result **out) {
    int32_t cluster, finish, isect;
    int64_t batch;
    std::string err;
    IsoFollow fol;
    if (!iso_options(options, &cluster, &finish, &batch, &isect, &err, &fol)) {
        if (out) *out = nullptr;
        return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, err);
    }
    return build_isosurfaces_impl(h, extents, resolution, isovalues, n_isovalues, drift, d_field_out, batch, cluster, finish, isect, out, fol);
}

int bbfmm_isosurfaces_from_values_opts(bbfmm_handle *h, const double *values, const double *extents, double resolution,
                                       const double *isovalues, int32_t n_isovalues,
                                       const bbfmm_isosurface_options *options, bbfmm_isosurface_result **out) {
    int32_t cluster, finish, isect;
    int64_t batch;
    std::string err;
    IsoFollow fol;
    if (!iso_options(options, &cluster, &finish, &batch, &isect, &err, &fol)) {
        if (out) *out = nullptr;
        return iso_fail(h, nullptr, BBFMM_BAD_ARGUMENT, err);
    }
    return isosurfaces_from_host(h, values, extents, resolution, isovalues, n_isovalues, batch, cluster, finish, isect, nullptr, 0,
                                 nullptr, 0, kIsoField, out, fol);
}

int bbfmm_isosurfaces_from_fields_opts(const bbfmm_field_operand *operands, int32_t n_operands, const int32_t *program,
                                       int32_t n_program, const double *extents, double resolution, const double *isovalues,
                                       int32_t n_isovalues, double *d_field_out, const bbfmm_isosurface_options *options,
                                       bbfmm_isosurface_result **out) {
    if (!out) return BBFMM_BAD_ARGUMENT;
    *out = nullptr;
    bbfmm_isosurface_result *r = nullptr;
    bbfmm_handle *h0 = nullptr; // the first operand with a handle: its stream and device, and a copy of the message
    try {
        r = new bbfmm_isosurface_result();
        *out = r;
        bbfmm::iso::Lattice lat;
        bbfmm::iso::Request req;
        std::string err;
        bool seed_gradients = false;
        int rc = field_request(extents, resolution, isovalues, n_isovalues, d_field_out, options, &lat, &req, &seed_gradients, &err);
        if (rc != BBFMM_OK) return iso_fail(nullptr, r, rc, err);
        CompositeField cf;
        if (!cf.setup(operands, n_operands, program, n_program, &err)) return iso_fail(nullptr, r, BBFMM_BAD_ARGUMENT, err);
        for (int o = 0; o < cf.n && !h0; ++o) h0 = cf.ops[o].h;
        if (h0) h0->err.clear();
        double box_lo[3], box_hi[3];
        for (int a = 0; a < 3; ++a) {
            box_lo[a] = lat.lo_world[a] + static_cast<double>(lat.lo[a]) * lat.spacing[a];
            box_hi[a] = lat.lo_world[a] + static_cast<double>(lat.lo[a] + lat.dims[a] - 1) * lat.spacing[a];
        }
        if ((rc = cf.inside(box_lo, box_hi, &err)) != BBFMM_OK) return iso_fail(h0, r, rc, err);
        // ---- device work from here
        OwnStream own;
        if (h0) {
            h0->tree.bind_device();
            cf.st = h0->tree.stream();
        } else {
            const hipError_t e = hipStreamCreateWithFlags(&own.st, hipStreamNonBlocking);
            if (e != hipSuccess) return iso_fail(h0, r, BBFMM_DEVICE_ERROR, std::string("isosurface: hipStreamCreate: ") + hipGetErrorString(e));
            cf.st = own.st;
        }
        for (int o = 0; o < cf.n; ++o)
            if (cf.ops[o].h && !cf.ops[o].ft.upload(cf.ops[o].h->tree))
                return iso_fail(h0, r, BBFMM_DEVICE_ERROR, "isosurface: operand " + std::to_string(o) + ": upload of the field terms");
        bbfmm::iso::FieldFn fn = [&cf](const double *x0, const double *x1, const double *x2, int64_t m, double *vals) {
            return cf.eval(x0, x1, x2, m, vals, nullptr);
        };
        if (seed_gradients && cf.gradients())
            req.grad = [&cf](const double *x0, const double *x1, const double *x2, int64_t m, double *vals, double *grad) {
                return cf.eval(x0, x1, x2, m, vals, grad);
            };
        rc = bbfmm::iso::extract(lat, fn, req, cf.st, &r->meshes, &err);
        if (rc != BBFMM_OK) {
            (void)hipStreamSynchronize(cf.st); // nothing of the call is queued when its columns are freed
            r->meshes.clear();
            return iso_fail(h0, r, rc, err.empty() ? cf.err : err);
        }
        return BBFMM_OK;
    } catch (const std::bad_alloc &) {
        return iso_fail(h0, r, BBFMM_BAD_ARGUMENT, "out of host memory");
    } catch (const std::exception &e) {
        return iso_fail(h0, r, BBFMM_BAD_ARGUMENT, std::string("exception: ") + e.what());
    }
}

int bbfmm_isosurfaces_from_function_opts(bbfmm_field_fn field, bbfmm_gradient_fn gradient, void *user, const double *extents,
                                         double resolution, const double *isovalues, int32_t n_isovalues,
                                         const bbfmm_isosurface_options *options, bbfmm_isosurface_result **out) {
    if (!out) return BBFMM_BAD_ARGUMENT;
    *out = nullptr;
    bbfmm_isosurface_result *r = nullptr;
    try {
        r = new bbfmm_isosurface_result();
        *out = r;
        if (!field) return iso_fail(nullptr, r, BBFMM_BAD_ARGUMENT, "isosurface: the field callback must not be null");
        bbfmm::iso::Lattice lat;
        bbfmm::iso::Request req;
        std::string err;
        bool seed_gradients = false;
        int rc = field_request(extents, resolution, isovalues, n_isovalues, nullptr, options, &lat, &req, &seed_gradients, &err);
        if (rc != BBFMM_OK) return iso_fail(nullptr, r, rc, err);
        OwnStream own;
        const hipError_t e = hipStreamCreateWithFlags(&own.st, hipStreamNonBlocking);
        if (e != hipSuccess) return iso_fail(nullptr, r, BBFMM_DEVICE_ERROR, std::string("isosurface: hipStreamCreate: ") + hipGetErrorString(e));
        FunctionField ff;
        ff.field = field;
        ff.gradient = gradient;
        ff.user = user;
        ff.st = own.st;
        bbfmm::iso::FieldFn fn = [&ff](const double *x0, const double *x1, const double *x2, int64_t m, double *vals) {
            return ff.eval(x0, x1, x2, m, vals, nullptr);
        };
        if (seed_gradients && gradient)
            req.grad = [&ff](const double *x0, const double *x1, const double *x2, int64_t m, double *vals, double *grad) {
                return ff.eval(x0, x1, x2, m, vals, grad);
            };
        rc = bbfmm::iso::extract(lat, fn, req, own.st, &r->meshes, &err);
        if (rc != BBFMM_OK) {
            (void)hipStreamSynchronize(own.st);
            r->meshes.clear();
            return iso_fail(nullptr, r, rc, err.empty() ? ff.err : err);
        }
        return BBFMM_OK;
    } catch (const std::bad_alloc &) {
        return iso_fail(nullptr, r, BBFMM_BAD_ARGUMENT, "out of host memory");
    } catch (const std::exception &e) {
        return iso_fail(nullptr, r, BBFMM_BAD_ARGUMENT, std::string("exception: ") + e.what());
    }
}

int bbfmm_debug_evaluate_fields(const bbfmm_field_operand *operands, int32_t n_operands, const int32_t *program, int32_t n_program,
                                const double *x, int64_t m, int64_t ldx, double *values, double *gradients, int64_t ldg) {
    bbfmm_handle *h0 = nullptr;
    try {
        CompositeField cf;
        std::string err;
        if (!cf.setup(operands, n_operands, program, n_program, &err)) {
            for (int o = 0; operands && o < cf.n && !h0; ++o) h0 = cf.ops[o].h;
            return iso_fail(h0, nullptr, BBFMM_BAD_ARGUMENT, err);
        }
        for (int o = 0; o < cf.n && !h0; ++o) h0 = cf.ops[o].h;
        if (h0) h0->err.clear();
        if (m < 0 || (m > 0 && (!x || !values || ldx < m || (gradients && ldg < m))))
            return iso_fail(h0, nullptr, BBFMM_BAD_ARGUMENT, "evaluate_fields: bad point or output arrays");
        if (gradients && !cf.gradients())
            return iso_fail(h0, nullptr, BBFMM_KERNEL_NO_GRADIENTS, "evaluate_fields: an operand's kernel does not support gradients");
        if (m == 0) return BBFMM_OK;
        OwnStream own;
        if (h0) {
            h0->tree.bind_device();
            cf.st = h0->tree.stream();
        } else {
            if (hipStreamCreateWithFlags(&own.st, hipStreamNonBlocking) != hipSuccess)
                return iso_fail(h0, nullptr, BBFMM_DEVICE_ERROR, "evaluate_fields: hipStreamCreate");
            cf.st = own.st;
        }
        for (int o = 0; o < cf.n; ++o)
            if (cf.ops[o].h && !cf.ops[o].ft.upload(cf.ops[o].h->tree))
                return iso_fail(h0, nullptr, BBFMM_DEVICE_ERROR, "evaluate_fields: operand " + std::to_string(o) + ": upload of the field terms");
        DevColumn dx, dv, dg;
        if (!dx.reserve(3 * m) || !dv.reserve(m) || (gradients && !dg.reserve(3 * m)))
            return iso_fail(h0, nullptr, BBFMM_DEVICE_ERROR, "evaluate_fields: out of device memory");
        const size_t bytes = static_cast<size_t>(m) * sizeof(double);
        hipError_t e = hipSuccess;
        for (int a = 0; a < 3 && e == hipSuccess; ++a) e = hipMemcpyAsync(dx.p + a * m, x + a * ldx, bytes, hipMemcpyHostToDevice, cf.st);
        if (e == hipSuccess) e = hipStreamSynchronize(cf.st);
        if (e != hipSuccess) return iso_fail(h0, nullptr, BBFMM_DEVICE_ERROR, std::string("evaluate_fields: upload of the points: ") + hipGetErrorString(e));
        int rc = cf.eval(dx.p, dx.p + m, dx.p + 2 * m, m, nullptr, nullptr); // every point inside every tree operand
        if (rc == BBFMM_OK) rc = cf.eval(dx.p, dx.p + m, dx.p + 2 * m, m, dv.p, gradients ? dg.p : nullptr);
        if (rc != BBFMM_OK) {
            (void)hipStreamSynchronize(cf.st);
            return iso_fail(h0, nullptr, rc, cf.err);
        }
        e = hipMemcpyAsync(values, dv.p, bytes, hipMemcpyDeviceToHost, cf.st);
        for (int a = 0; a < 3 && gradients && e == hipSuccess; ++a)
            e = hipMemcpyAsync(gradients + a * ldg, dg.p + a * m, bytes, hipMemcpyDeviceToHost, cf.st);
        if (e == hipSuccess) e = hipStreamSynchronize(cf.st);
        if (e != hipSuccess) return iso_fail(h0, nullptr, BBFMM_DEVICE_ERROR, std::string("evaluate_fields: download: ") + hipGetErrorString(e));
        return BBFMM_OK;
    } catch (const std::bad_alloc &) {
        return iso_fail(h0, nullptr, BBFMM_BAD_ARGUMENT, "out of host memory");
    } catch (const std::exception &e) {
        return iso_fail(h0, nullptr, BBFMM_BAD_ARGUMENT, std::string("exception: ") + e.what());
    }
}

int bbfmm_debug_field_program(int32_t where, int32_t n_operands, const double *scale, const double *offset, const int32_t *program,
                              int32_t n_program, const double *V, const double *G, int64_t m, double *out_v, double *out_g) {
    bbfmm::FieldProgram p;
    std::string err;
    if ((where != 0 && where != 1) || m < 0 || !bbfmm::field_program_make(n_operands, scale, offset, program, n_program, &p, &err))
        return BBFMM_BAD_ARGUMENT;
    if (m == 0) return BBFMM_OK;
    if (!V || !out_v || (G && !out_g)) return BBFMM_BAD_ARGUMENT;
    if (where == 1) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return BBFMM_DEVICE_ERROR;
        try {
            return bbfmm::field_program_debug_device(p, V, G, m, out_v, out_g) == 0 ? BBFMM_OK : BBFMM_DEVICE_ERROR;
        } catch (...) {
            return BBFMM_BAD_ARGUMENT;
        }
    }
    bbfmm::FieldColumns c;
    for (int o = 0; o < p.n_operands; ++o) {
        c.v[o] = V + static_cast<size_t>(o) * m;
        c.g[o] = G ? G + static_cast<size_t>(3 * o) * m : nullptr;
        c.ldg[o] = m;
    }
    for (int64_t i = 0; i < m; ++i) {
        double g[3];
        bbfmm::field_program_node(p, c, i, &out_v[i], G ? g : nullptr);
        if (G)
            for (int a = 0; a < 3; ++a) out_g[static_cast<size_t>(a) * m + i] = g[a];
    }
    return BBFMM_OK;
}

int bbfmm_isosurface_finish_mesh(bbfmm_handle *h, const double *vertices, int64_t n_vertices, const int64_t *facets,
                                 int64_t n_facets, const double *extents, bbfmm_isosurface_result **out) {
    return isosurfaces_from_host(h, nullptr, extents, 0.0, nullptr, 0, 0, BBFMM_CLUSTER_NONE, BBFMM_FINISH_CLIPPED,
                                 BBFMM_SELF_INTERSECTIONS_IGNORE, vertices, n_vertices, facets, n_facets, kIsoFinishMesh, out);
}

int bbfmm_isosurface_close_mesh(bbfmm_handle *h, const double *vertices, int64_t n_vertices, const int64_t *facets,
                                int64_t n_facets, const double *extents, double resolution, int32_t mode,
                                bbfmm_isosurface_result **out) {
    return isosurfaces_from_host(h, nullptr, extents, resolution, nullptr, 0, 0, BBFMM_CLUSTER_NONE, mode,
                                 BBFMM_SELF_INTERSECTIONS_IGNORE, vertices, n_vertices, facets, n_facets, kIsoCloseMesh, out);
}

int bbfmm_isosurface_closure_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out) {
    if (!r || !stats_out || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    static_assert(sizeof(r->meshes[i].closure_stats) == BBFMM_CLOSURE_STATS * sizeof(int64_t), "closure stats");
    std::memcpy(stats_out, r->meshes[i].closure_stats, sizeof(r->meshes[i].closure_stats));
    return BBFMM_OK;
}

int bbfmm_debug_orient2d(const double *abc, int64_t n, int32_t *sign_out) {
    if (n < 0 || (n > 0 && (!abc || !sign_out))) return BBFMM_BAD_ARGUMENT;
    for (int64_t i = 0; i < n; ++i) sign_out[i] = bbfmm::iso::closure::orient2d_sign(abc + 6 * i, abc + 6 * i + 2, abc + 6 * i + 4);
    return BBFMM_OK;
}

int bbfmm_debug_closure_triangulate(int32_t nu, int32_t nv, const double *gu, const double *gv, const double *points,
                                    int64_t n_points, const int64_t *edges, int64_t n_edges, const int32_t *cut,
                                    int64_t n_cut, double tol, double key_cell, int64_t cap_points, double *pts_out,
                                    int64_t *ids_out, int64_t cap_tris, int64_t *tris_out, int64_t *counts_out,
                                    char *err_out, int64_t err_cap) {
    auto fail = [&](const std::string &msg) {
        if (err_out && err_cap > 0) {
            const size_t n = std::min(msg.size(), static_cast<size_t>(err_cap - 1));
            std::memcpy(err_out, msg.data(), n);
            err_out[n] = 0;
        }
        return BBFMM_BAD_ARGUMENT;
    };
    try {
        if (nu < 1 || nv < 1 || !gu || !gv || n_points < 0 || n_edges < 0 || n_cut < 0 || (n_points > 0 && !points) ||
            (n_edges > 0 && !edges) || (n_cut > 0 && !cut) || !counts_out || cap_points < 0 || cap_tris < 0 || !(key_cell > 0.0) ||
            n_points > 2000000000 || n_cut > 400000000)
            return fail("closure: bad arguments");
        bbfmm::iso::closure::Band B;
        B.nu = nu, B.nv = nv, B.gu = gu, B.gv = gv, B.points = points, B.n_points = n_points, B.edges = edges, B.n_edges = n_edges;
        B.cut = cut, B.n_cut = n_cut, B.tol = tol, B.key_cell = key_cell;
        std::string err;
        if (!bbfmm::iso::closure::triangulate_band(&B, &err)) return fail(err);
        const int64_t np = static_cast<int64_t>(B.id.size()), nt = static_cast<int64_t>(B.tri.size() / 3);
        if (np > cap_points || nt > cap_tris || (np > 0 && (!pts_out || !ids_out)) || (nt > 0 && !tris_out))
            return fail("closure: " + std::to_string(np) + " band points and " + std::to_string(nt) + " triangles do not fit the capacities given");
        if (np) std::memcpy(pts_out, B.xy.data(), B.xy.size() * sizeof(double));
        if (np) std::memcpy(ids_out, B.id.data(), B.id.size() * sizeof(int64_t));
        if (nt) std::memcpy(tris_out, B.tri.data(), B.tri.size() * sizeof(int64_t));
        for (int q = 0; q < 8; ++q) counts_out[q] = 0;
        counts_out[0] = np, counts_out[1] = nt, counts_out[2] = B.dropped, counts_out[3] = B.constraint_flips, counts_out[4] = B.lawson_flips;
        return BBFMM_OK;
    } catch (const std::exception &e) {
        return fail(std::string("exception: ") + e.what());
    }
}

int bbfmm_isosurface_self_intersections(bbfmm_handle *h, const double *vertices, int64_t n_vertices, const int64_t *facets,
                                        int64_t n_facets, const double *extents, bbfmm_isosurface_result **out) {
    return isosurfaces_from_host(h, nullptr, extents, 0.0, nullptr, 0, 0, BBFMM_CLUSTER_NONE, BBFMM_FINISH_RAW,
                                 BBFMM_SELF_INTERSECTIONS_IGNORE, vertices, n_vertices, facets, n_facets, kIsoDetectMesh, out);
}

int bbfmm_isosurface_intersection_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out) {
    if (!r || !stats_out || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    std::memcpy(stats_out, r->meshes[i].isect_stats, sizeof(r->meshes[i].isect_stats));
    return BBFMM_OK;
}

int bbfmm_isosurface_intersection_ids(const bbfmm_isosurface_result *r, int32_t i, int64_t *n_ids_out, int64_t *ids_out) {
    if (!r || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    const std::vector<int64_t> &ids = r->meshes[i].isect_ids;
    if (n_ids_out) *n_ids_out = static_cast<int64_t>(ids.size());
    if (ids_out && !ids.empty()) std::memcpy(ids_out, ids.data(), ids.size() * sizeof(int64_t));
    return BBFMM_OK;
}

int bbfmm_isosurface_triangle_pair(const double *tri_a, const int64_t *ids_a, const double *tri_b, const int64_t *ids_b,
                                   int32_t *result_out, int32_t *stage_out) {
    using namespace bbfmm::iso;
    if (!tri_a || !ids_a || !tri_b || !ids_b || !result_out) return BBFMM_BAD_ARGUMENT;
    Tri3 a, b;
    for (int k = 0; k < 3; ++k)
        for (int x = 0; x < 3; ++x) {
            a.p[k].x[x] = tri_a[3 * k + x];
            b.p[k].x[x] = tri_b[3 * k + x];
        }
    int stage = 0;
    *result_out = triangle_pair(a, ids_a, b, ids_b, &stage) ? 1 : 0;
    if (stage_out) *stage_out = stage;
    return BBFMM_OK;
}

int bbfmm_isosurface_follow_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out) {
    if (!r || !stats_out || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    std::memcpy(stats_out, r->meshes[i].follow_stats, sizeof(r->meshes[i].follow_stats));
    return BBFMM_OK;
}

int bbfmm_isosurface_follow_bricks(const bbfmm_isosurface_result *r, int32_t i, int32_t *dims_out, uint8_t *bricks_out) {
    if (!r || !dims_out || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    const bbfmm::iso::Mesh &m = r->meshes[i];
    std::memcpy(dims_out, m.follow_dims, sizeof(m.follow_dims));
    if (bricks_out && !m.follow_bricks.empty()) std::memcpy(bricks_out, m.follow_bricks.data(), m.follow_bricks.size());
    return BBFMM_OK;
}

int bbfmm_isosurface_follow_times(const bbfmm_isosurface_result *r, int32_t i, double *ms_out) {
    if (!r || !ms_out || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    std::memcpy(ms_out, r->meshes[i].follow_ms, sizeof(r->meshes[i].follow_ms));
    return BBFMM_OK;
}

int bbfmm_isosurface_curvature_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out) {
    if (!r || !stats_out || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    std::memcpy(stats_out, r->meshes[i].curv_stats, sizeof(r->meshes[i].curv_stats));
    return BBFMM_OK;
}

int bbfmm_isosurface_finish_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out) {
    if (!r || !stats_out || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    std::memcpy(stats_out, r->meshes[i].finish_stats, sizeof(r->meshes[i].finish_stats));
    return BBFMM_OK;
}

int bbfmm_isosurface_clip_triangle(const double *triangle, const double *extents, double *points_out, int32_t *corner_out,
                                   int32_t *n_points_out) {
    using namespace bbfmm::iso;
    if (!triangle || !points_out || !n_points_out) return BBFMM_BAD_ARGUMENT;
    ClipBox box;
    std::string err;
    if (!make_clip_box(extents, &box, &err)) return BBFMM_BAD_ARGUMENT;
    double tri[3][3], pts[kClipMaxPoints][3];
    int corner[kClipMaxPoints];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) tri[k][a] = triangle[3 * k + a];
    const int n = clip_triangle(tri, box, pts, corner);
    *n_points_out = n;
    for (int k = 0; k < n; ++k) {
        for (int a = 0; a < 3; ++a) points_out[3 * k + a] = pts[k][a];
        if (corner_out) corner_out[k] = corner[k];
    }
    return BBFMM_OK;
}

int bbfmm_isosurfaces_from_values(bbfmm_handle *h, const double *values, const double *extents, double resolution,
                                  const double *isovalues, int32_t n_isovalues, int64_t batch_bytes,
                                  bbfmm_isosurface_result **out) {
    return bbfmm_isosurfaces_from_values_ex(h, values, extents, resolution, isovalues, n_isovalues, batch_bytes,
                                            BBFMM_CLUSTER_NONE, out);
}

int bbfmm_isosurfaces_from_values_ex(bbfmm_handle *h, const double *values, const double *extents, double resolution,
                                     const double *isovalues, int32_t n_isovalues, int64_t batch_bytes,
                                     int32_t cluster_method, bbfmm_isosurface_result **out) {
    return isosurfaces_from_host(h, values, extents, resolution, isovalues, n_isovalues, batch_bytes, cluster_method, BBFMM_FINISH_RAW,
                                 BBFMM_SELF_INTERSECTIONS_IGNORE, nullptr, 0, nullptr, 0, kIsoField, out);
}

int32_t bbfmm_isosurface_count(const bbfmm_isosurface_result *r) { return r ? static_cast<int32_t>(r->meshes.size()) : -1; }

int bbfmm_isosurface_size(const bbfmm_isosurface_result *r, int32_t i, int64_t *n_vertices, int64_t *n_facets) {
    if (!r || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    if (n_vertices) *n_vertices = static_cast<int64_t>(r->meshes[i].vertices.size() / 3);
    if (n_facets) *n_facets = static_cast<int64_t>(r->meshes[i].facets.size() / 3);
    return BBFMM_OK;
}

int bbfmm_isosurface_copy(const bbfmm_isosurface_result *r, int32_t i, double *vertices, int64_t *facets) {
    if (!r || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    const bbfmm::iso::Mesh &m = r->meshes[i];
    if ((!vertices && !m.vertices.empty()) || (!facets && !m.facets.empty())) return BBFMM_BAD_ARGUMENT;
    if (!m.vertices.empty()) std::memcpy(vertices, m.vertices.data(), m.vertices.size() * sizeof(double));
    if (!m.facets.empty()) std::memcpy(facets, m.facets.data(), m.facets.size() * sizeof(int64_t));
    return BBFMM_OK;
}

int bbfmm_isosurface_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out) {
    if (!r || !stats_out || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    std::memcpy(stats_out, r->meshes[i].stats, sizeof(r->meshes[i].stats));
    return BBFMM_OK;
}

const char *bbfmm_isosurface_error(const bbfmm_isosurface_result *r) { return r ? r->err.c_str() : "null result"; }

void bbfmm_isosurface_destroy(bbfmm_isosurface_result *r) { delete r; }

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
    if (h->group) {
        h->err = "the handle spans a device group: its partition is the group's";
        return BBFMM_BAD_ARGUMENT;
    }
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
    if (h->group) {
        h->err = "the handle spans a device group: the exchange is the library's";
        return BBFMM_BAD_ARGUMENT;
    }
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
    if (h->group) {
        h->err = "the handle spans a device group: the exchange is the library's";
        return BBFMM_BAD_ARGUMENT;
    }
    return h->tree.matvec_partition_finish_sorted(d_coarse, d_seg, ld, static_cast<hipStream_t>(comm_stream));
    END_GUARD(h)
}
int bbfmm_partition_scatter(bbfmm_handle *h, const double *d_all, int32_t first_part, int32_t n_parts, int64_t m_max, int32_t k,
                            double *d_out, int64_t ldo) {
    GUARD(h)
    if (h->group) {
        h->err = "the handle spans a device group: the exchange is the library's";
        return BBFMM_BAD_ARGUMENT;
    }
    return h->tree.partition_scatter(d_all, first_part, n_parts, m_max, k, d_out, ldo);
    END_GUARD(h)
}
int bbfmm_matvec_partition_finish(bbfmm_handle *h, const double *d_coarse, double *d_out, int64_t ldo, int32_t sync, void *comm_stream) {
    GUARD(h)
    if (h->group) {
        h->err = "the handle spans a device group: the exchange is the library's";
        return BBFMM_BAD_ARGUMENT;
    }
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

// ------------------------------------------------------------------ domain decomposition (host part)
#include "ddm.hpp"
struct bbfmm_ddm {
    bbfmm::DdmTree tree;
};
extern "C" {
void bbfmm_ddm_params_defaults(bbfmm_ddm_params *out) {
    if (!out) return;
    const bbfmm::DdmParams p;
    out->leaf_threshold = p.leaf_threshold;
    out->overlap_quota = p.overlap_quota;
    out->coarse_ratio = p.coarse_ratio;
    out->coarse_threshold = p.coarse_threshold;
}

void bbfmm_ddm_params_for_points(int64_t n, bbfmm_ddm_params *out) {
    if (!out) return;
    bbfmm_ddm_params_defaults(out);
    // per level at most N (1/8 + 1/341) points survive (rounding up per leaf, leaves of more than 341 points)
    out->coarse_threshold = std::max<int64_t>(out->coarse_threshold, n / 470 + 1);
}
int bbfmm_ddm_build(const double *points, int64_t n, int32_t d, int64_t ld, const bbfmm_ddm_params *params,
                    bbfmm_ddm **out) {
    if (!out) return BBFMM_BAD_ARGUMENT;
    *out = nullptr;
    bbfmm::DdmParams p;
    if (params) {
        p.leaf_threshold = params->leaf_threshold;
        p.overlap_quota = params->overlap_quota;
        p.coarse_ratio = params->coarse_ratio;
        p.coarse_threshold = params->coarse_threshold;
    }
    bbfmm_ddm *t = new (std::nothrow) bbfmm_ddm();
    if (!t) return BBFMM_DEVICE_ERROR;
    int rc = BBFMM_BAD_ARGUMENT;
    try {
        rc = bbfmm::build_ddm_tree(points, n, d, ld, p, &t->tree);
    } catch (...) {
        rc = BBFMM_DEVICE_ERROR;
    }
    if (rc != BBFMM_OK) {
        delete t;
        return rc;
    }
    *out = t;
    return BBFMM_OK;
}
void bbfmm_ddm_destroy(bbfmm_ddm *t) { delete t; }
int32_t bbfmm_ddm_num_levels(const bbfmm_ddm *t) { return t ? static_cast<int32_t>(t->tree.levels.size()) : 0; }
static const bbfmm::DdmLevel *ddm_level(const bbfmm_ddm *t, int32_t level) {
    if (!t || level < 0 || level >= static_cast<int32_t>(t->tree.levels.size())) return nullptr;
    return &t->tree.levels[static_cast<size_t>(level)];
}
int64_t bbfmm_ddm_level_size(const bbfmm_ddm *t, int32_t level) {
    const bbfmm::DdmLevel *l = ddm_level(t, level);
    return l ? static_cast<int64_t>(l->point_indices.size()) : -1;
}
int bbfmm_ddm_level_points(const bbfmm_ddm *t, int32_t level, int64_t *out) {
    const bbfmm::DdmLevel *l = ddm_level(t, level);
    if (!l || !out) return BBFMM_BAD_ARGUMENT;
    std::copy(l->point_indices.begin(), l->point_indices.end(), out);
    return BBFMM_OK;
}
int64_t bbfmm_ddm_num_domains(const bbfmm_ddm *t, int32_t level) {
    const bbfmm::DdmLevel *l = ddm_level(t, level);
    return l ? static_cast<int64_t>(l->leaves.size()) : -1;
}
int64_t bbfmm_ddm_domain_size(const bbfmm_ddm *t, int32_t level, int64_t domain) {
    const bbfmm::DdmLevel *l = ddm_level(t, level);
    if (!l || domain < 0 || domain >= static_cast<int64_t>(l->leaves.size())) return -1;
    return static_cast<int64_t>(l->leaves[static_cast<size_t>(domain)].idx.size());
}
int bbfmm_ddm_domain(const bbfmm_ddm *t, int32_t level, int64_t domain, int64_t *indices, uint8_t *internal,
                     double *extents) {
    const bbfmm::DdmLevel *l = ddm_level(t, level);
    if (!l || domain < 0 || domain >= static_cast<int64_t>(l->leaves.size())) return BBFMM_BAD_ARGUMENT;
    const bbfmm::DdmDomain &dm = l->leaves[static_cast<size_t>(domain)];
    if (indices) std::copy(dm.idx.begin(), dm.idx.end(), indices);
    if (internal) std::copy(dm.internal.begin(), dm.internal.end(), internal);
    if (extents) std::copy(dm.extents.begin(), dm.extents.end(), extents);
    return BBFMM_OK;
}
} // extern "C"

// ---- evaluation at device targets and on regular grids (fmm_tree.hpp evaluate_device, evaluate_grid.hpp)
namespace {

struct EvalOptions {
    bool batch_independent = false;
    int32_t cap = 0;
    int64_t batch_bytes = 0;
    bool outputs_on_device = false;
};

// The fields of *o that its size covers; defaults for the rest and for o == nullptr.
bool eval_options(const bbfmm_evaluate_options *o, const FmmTree &tree, EvalOptions *out, std::string *err) {
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

// Device memory of one call, freed on every exit.
struct DevDoubles {
    double *p = nullptr;
    ~DevDoubles() { (void)hipFree(p); }
    bool get(size_t n) { return hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(n, 1) * sizeof(double)) == hipSuccess; }
};

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
    FmmTree &tree = h->tree;
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
    DevDoubles x, vals, grads;
    const bool stage = !eo.outputs_on_device;
    if (!x.get(static_cast<size_t>(slab_cap) * d) || (stage && !vals.get(static_cast<size_t>(slab_cap) * k)) ||
        (stage && with_gradients && !grads.get(static_cast<size_t>(slab_cap) * k * d)))
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
    DevDoubles x;
    if (!x.get(static_cast<size_t>(n) * g.d) || bbfmm::grid_coords_device(g, r0, n, x.p, n, nullptr) != 0 ||
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
    struct Mem {
        void *p = nullptr;
        ~Mem() { (void)hipFree(p); }
    } mem;
    const size_t temp_off = (ints * sizeof(int32_t) + 255) & ~size_t(255);
    if (hipMalloc(&mem.p, temp_off + std::max<size_t>(temp_bytes, 1)) != hipSuccess) return BBFMM_DEVICE_ERROR;
    int32_t *base = static_cast<int32_t *>(mem.p);
    int32_t *d_jc = base, *d_tb = base + nr, *d_te = base + 2 * nr, *d_cnt = base + 3 * nr, *d_offs = base + 4 * nr;
    int32_t *o_jc = base + 5 * nr, *o_tb = o_jc + jcap, *o_te = o_tb + jcap, *d_n = o_te + jcap;
    if (hipMemcpy(d_jc, job_cell, nr * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_tb, tgt_begin, nr * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_te, tgt_end, nr * 4, hipMemcpyHostToDevice) != hipSuccess)
        return BBFMM_DEVICE_ERROR;
    if (bbfmm::split_runs(d_jc, d_tb, d_te, n_runs, cap, d_cnt, d_offs, o_jc, o_tb, o_te, static_cast<int64_t>(jcap), d_n, static_cast<uint8_t *>(mem.p) + temp_off, temp_bytes,
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
