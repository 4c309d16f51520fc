// extern "C" boundary: isosurfaces of composite fields and of callers' functions (field_program.hpp; DESIGN.md
// "Composite fields"), over what capi_isosurface.hpp shares with the entries of a single tree.
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "capi_isosurface.hpp"
#include "field_program.hpp"

namespace {

struct FieldOperand {
    int kind = BBFMM_FIELD_AFFINE, axis = 2;
    bbfmm_handle *h = nullptr;
    IsoFieldTerms ft;
    double affine[4] = {0, 0, 0, 0};
    bbfmm::DevBuffer<> v, g; // the operand's values and, for the seed projection, its 3 gradient columns
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
            const int rc = iso_box_in_tree(op.h->tree, lo, hi, "isosurface: operand " + std::to_string(o) + ": ", "its ", msg);
            if (rc != BBFMM_OK) return rc;
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
    iso_fill_request(req, isovalues, n_isovalues, d_field_out, batch, cluster, finish, extents, isect, fol);
    *seed_gradients = false;
    if (fol.follow == BBFMM_FOLLOW_SURFACE && !iso_seed_gradients(seed_gradients, err)) return BBFMM_BAD_ARGUMENT;
    return BBFMM_OK;
}

} // namespace

extern "C" {

int bbfmm_isosurfaces_from_fields_opts(const bbfmm_field_operand *operands, int32_t n_operands, const int32_t *program,
                                       int32_t n_program, const double *extents, double resolution, const double *isovalues,
                                       int32_t n_isovalues, double *d_field_out, const bbfmm_isosurface_options *options,
                                       bbfmm_isosurface_result **out) {
    if (!out) return BBFMM_BAD_ARGUMENT;
    bbfmm_handle *h0 = nullptr; // the first operand with a handle: its stream and device, and a copy of the message
    return iso_with_result(&h0, out, [&](bbfmm_isosurface_result *r) -> int {
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
        lat.node_box(box_lo, box_hi);
        if ((rc = cf.inside(box_lo, box_hi, &err)) != BBFMM_OK) return iso_fail(h0, r, rc, err);
        // ---- device work from here
        bbfmm::OwnStream own;
        if (h0) {
            h0->tree.bind_device();
            cf.st = h0->tree.stream();
        } else {
            const hipError_t e = own.create();
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
    });
}

int bbfmm_isosurfaces_from_function_opts(bbfmm_field_fn field, bbfmm_gradient_fn gradient, void *user, const double *extents,
                                         double resolution, const double *isovalues, int32_t n_isovalues,
                                         const bbfmm_isosurface_options *options, bbfmm_isosurface_result **out) {
    if (!out) return BBFMM_BAD_ARGUMENT;
    bbfmm_handle *const no_handle = nullptr;
    return iso_with_result(&no_handle, out, [&](bbfmm_isosurface_result *r) -> int {
        if (!field) return iso_fail(nullptr, r, BBFMM_BAD_ARGUMENT, "isosurface: the field callback must not be null");
        bbfmm::iso::Lattice lat;
        bbfmm::iso::Request req;
        std::string err;
        bool seed_gradients = false;
        int rc = field_request(extents, resolution, isovalues, n_isovalues, nullptr, options, &lat, &req, &seed_gradients, &err);
        if (rc != BBFMM_OK) return iso_fail(nullptr, r, rc, err);
        bbfmm::OwnStream own;
        const hipError_t e = own.create();
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
    });
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
        bbfmm::OwnStream own;
        if (h0) {
            h0->tree.bind_device();
            cf.st = h0->tree.stream();
        } else {
            if (own.create() != hipSuccess)
                return iso_fail(h0, nullptr, BBFMM_DEVICE_ERROR, "evaluate_fields: hipStreamCreate");
            cf.st = own.st;
        }
        for (int o = 0; o < cf.n; ++o)
            if (cf.ops[o].h && !cf.ops[o].ft.upload(cf.ops[o].h->tree))
                return iso_fail(h0, nullptr, BBFMM_DEVICE_ERROR, "evaluate_fields: operand " + std::to_string(o) + ": upload of the field terms");
        bbfmm::DevBuffer<> dx, dv, dg;
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

} // extern "C"
