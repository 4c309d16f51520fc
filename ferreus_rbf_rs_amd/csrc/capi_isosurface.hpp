// What the isosurface entries (capi_isosurface.cpp) share with those of composite fields and callers' functions
// (capi_fields.cpp): the result object, the checked options and the field terms of one interpolant on the device.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "capi_handle.hpp"
#include "interpolant_terms.hpp"
#include "isosurface.hpp"

struct bbfmm_isosurface_result {
    std::vector<bbfmm::iso::Mesh> meshes;
    std::string err;
};

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
    bbfmm::DevBuffer<> d_lambda, xt[3];
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
    bool upload(bbfmm::FmmTree &tree) {
        if (!on) return true;
        tree.bind_device();
        const int nb = bbfmm::terms_basis_size(t.d, t.degree);
        if (nb > 0) {
            if (!d_lambda.reserve(nb) || hipMemcpy(d_lambda.p, t.lambda, nb * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
                return false;
            t.lambda = d_lambda.p;
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
    int eval(bbfmm::FmmTree &tree, const double *x0, const double *x1, const double *x2, int64_t m, double *vals, double *grad) {
        int64_t bad = -1;
        if (!on) return tree.evaluate_leaves_device(x0, x1, x2, m, vals, &bad, grad);
        const double *q[3] = {x0, x1, x2};
        if (t.has_affine && m > 0) {
            if (!xt[0].reserve(m) || !xt[1].reserve(m) || !xt[2].reserve(m)) return BBFMM_DEVICE_ERROR;
            if (bbfmm::terms_affine_soa_device(t, x0, x1, x2, m, xt[0].p, xt[1].p, xt[2].p, tree.stream()) != 0) return BBFMM_DEVICE_ERROR;
            for (int a = 0; a < t.d; ++a) q[a] = xt[a].p;
        }
        // a deterministic handle gets the same double in every batching; a default one has f64 atomics between its M2P
        // jobs anyway and keeps the tuned plan
        const int rc = tree.evaluate_leaves_device(q[0], q[1], q[2], m, vals, &bad, grad, tree.deterministic());
        if (rc != BBFMM_OK || !vals) return rc;
        return bbfmm::terms_field_soa_device(t, x0, x1, x2, m, vals, grad, tree.stream()) == 0 ? BBFMM_OK : BBFMM_DEVICE_ERROR;
    }
};

// Arguments shared by the extraction entry points; false with *err set on a bad one.
bool iso_args(const double *extents, double resolution, const double *isovalues, int32_t n_iso, bbfmm::iso::Lattice *lat, std::string *err);
bool iso_options(const bbfmm_isosurface_options *o, int32_t *cluster, int32_t *finish, int64_t *batch_bytes, int32_t *self_intersections,
                 std::string *err, IsoFollow *fol = nullptr);
bool iso_follow_ok(const IsoFollow &fol, bool need_seeds, std::string *err);
bool iso_methods_ok(int32_t cluster, int32_t finish, int32_t self_intersections, std::string *err);
// BBFMM_ISO_SEED_GRADIENTS (read per call): `differences` takes the reference's central differences of the values
// (seed_projection.rs:138-189), which a kernel without gradients takes anyway; `leaf_pass`, empty or unset: the field's own
// gradients (*own).  false with *err set for anything else.
bool iso_seed_gradients(bool *own, std::string *err);
// The message of a failure for the handle and the result (either may be null); returns rc.
int iso_fail(bbfmm_handle *h, bbfmm_isosurface_result *r, int rc, const std::string &msg);
// What every extraction asks of extract(); the seeds of fol only with BBFMM_FOLLOW_SURFACE.  Everything else keeps its default.
void iso_fill_request(bbfmm::iso::Request *req, const double *isovalues, int32_t n_isovalues, double *d_field_out, int64_t batch_bytes,
                      int32_t cluster, int32_t finish, const double *extents, int32_t self_intersections, const IsoFollow &fol);
// Every node of a lattice box [lo, hi] (the tree's own axes) inside the tree's cube: points_to_leaves saturates
// coordinates below the tree, as the reference's Morton encoding does, so the bounds are checked before any evaluation.
// BBFMM_POINT_OUTSIDE_TREE with *msg = at + "lattice nodes on " + its + "axis ..." otherwise.
int iso_box_in_tree(const bbfmm::FmmTree &tree, const double *lo, const double *hi, const std::string &at, const char *its, std::string *msg);

// An entry that owns its result: *out receives it before anything else can fail (the message of a failure is read from
// it), body(r) does the work, and running out of host memory or an exception becomes the message of r and of *h.
template <class Body>
int iso_with_result(bbfmm_handle *const *h, bbfmm_isosurface_result **out, Body &&body) {
    *out = nullptr;
    bbfmm_isosurface_result *r = nullptr;
    try {
        r = new bbfmm_isosurface_result();
        *out = r;
        return body(r);
    } catch (const std::bad_alloc &) {
        return iso_fail(*h, r, BBFMM_BAD_ARGUMENT, "out of host memory");
    } catch (const std::exception &e) {
        return iso_fail(*h, r, BBFMM_BAD_ARGUMENT, std::string("exception: ") + e.what());
    }
}
