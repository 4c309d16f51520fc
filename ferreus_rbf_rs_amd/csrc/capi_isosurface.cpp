// extern "C" boundary: isosurfaces of one tree's interpolant or of a caller's values, the mesh entries (clip and clean,
// closure, self-intersections), the getters of a result and the hooks of the isosurface tables (isosurface.hpp).
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "capi_isosurface.hpp"
#include "closure_triangulate.hpp"
#include "isosurface_closure.hpp"
#include "isosurface_curvature.hpp"
#include "isosurface_intersect.hpp"

using bbfmm::FmmTree;

bool iso_args(const double *extents, double resolution, const double *isovalues, int32_t n_iso, bbfmm::iso::Lattice *lat, std::string *err) {
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

bool iso_options(const bbfmm_isosurface_options *o, int32_t *cluster, int32_t *finish, int64_t *batch_bytes, int32_t *self_intersections,
                 std::string *err, IsoFollow *fol) {
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

bool iso_follow_ok(const IsoFollow &fol, bool need_seeds, std::string *err) {
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

bool iso_methods_ok(int32_t cluster, int32_t finish, int32_t self_intersections, std::string *err) {
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

bool iso_seed_gradients(bool *own, std::string *err) {
    const char *sg = std::getenv("BBFMM_ISO_SEED_GRADIENTS");
    if (sg && *sg && std::strcmp(sg, "differences") != 0 && std::strcmp(sg, "leaf_pass") != 0) {
        *err = std::string("isosurface: BBFMM_ISO_SEED_GRADIENTS must be leaf_pass or differences, got '") + sg + "'";
        return false;
    }
    *own = !(sg && !std::strcmp(sg, "differences"));
    return true;
}

int iso_fail(bbfmm_handle *h, bbfmm_isosurface_result *r, int rc, const std::string &msg) {
    if (h) h->err = msg;
    if (r) r->err = msg;
    return rc;
}

void iso_fill_request(bbfmm::iso::Request *req, const double *isovalues, int32_t n_isovalues, double *d_field_out, int64_t batch_bytes,
                      int32_t cluster, int32_t finish, const double *extents, int32_t self_intersections, const IsoFollow &fol) {
    req->isovalues = isovalues;
    req->n_iso = n_isovalues;
    req->d_field_out = d_field_out;
    req->budget_bytes = batch_bytes;
    req->cluster = cluster;
    req->finish = finish;
    req->extents = extents;
    req->self_intersections = self_intersections;
    req->follow = fol.follow;
    if (fol.follow == BBFMM_FOLLOW_SURFACE) {
        req->seeds = fol.seeds;
        req->n_seeds = fol.n_seeds;
        req->seeds_ld = fol.seeds_ld;
    }
}

int iso_box_in_tree(const FmmTree &tree, const double *lo, const double *hi, const std::string &at, const char *its, std::string *msg) {
    const auto &tr = tree.tree();
    for (int a = 0; a < tr.d; ++a)
        if (!(lo[a] >= tr.center[a] - tr.radius) || !(hi[a] <= tr.center[a] + tr.radius)) {
            *msg = at + "lattice nodes on " + its + "axis " + std::to_string(a) + " span [" + std::to_string(lo[a]) + ", " +
                   std::to_string(hi[a]) + "], outside the tree extents [" + std::to_string(tr.center[a] - tr.radius) + ", " +
                   std::to_string(tr.center[a] + tr.radius) + "] (pad the tree's extents, as rbf.rs:992-998 does)";
            return BBFMM_POINT_OUTSIDE_TREE;
        }
    return BBFMM_OK;
}

// A getter of mesh i: the bounds check and the copy of one fixed-size member.
template <class Member>
static int mesh_member(const bbfmm_isosurface_result *r, int32_t i, void *out, Member bbfmm::iso::Mesh::*member) {
    if (!r || !out || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    std::memcpy(out, &(r->meshes[i].*member), sizeof(Member));
    return BBFMM_OK;
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
    // every node of E inside the tree's cube: the device pass of extract() then finds every leaf.
    // With a global trend: the extents of the 8 transformed corners of the lattice box (rbf.rs:599-613).
    double box_lo[3], box_hi[3];
    lat.node_box(box_lo, box_hi);
    ft.tree_box(box_lo, box_hi);
    if (iso_box_in_tree(t, box_lo, box_hi, "isosurface: ", "", &err) != BBFMM_OK) return iso_fail(h, nullptr, BBFMM_POINT_OUTSIDE_TREE, err);
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
    iso_fill_request(&req, isovalues, n_isovalues, d_field_out, batch_bytes, cluster_method, finish, extents, self_intersections, fol);
    req.drift = drift;
    if (fol.follow == BBFMM_FOLLOW_SURFACE) {
        if (!fol.seeds) { // the data points (rbf.rs:1049)
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
    return iso_with_result(&h, out, [&](bbfmm_isosurface_result *r) -> int {
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
        bbfmm::OwnStream own;
        if (!h) {
            const hipError_t e = own.create();
            if (e != hipSuccess) return iso_fail(h, r, BBFMM_DEVICE_ERROR, std::string("isosurface: hipStreamCreate: ") + hipGetErrorString(e));
        }
        const hipStream_t st = h ? h->tree.stream() : own.st;
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
            iso_fill_request(&req, isovalues, n_isovalues, nullptr, batch_bytes, cluster_method, finish, extents, self_intersections, fol);
            req.host_field = values;
            req.seeds = fol.seeds; // (whatever the follow mode)
            req.n_seeds = fol.n_seeds;
            req.seeds_ld = fol.seeds_ld;
            rc = bbfmm::iso::extract(lat, bbfmm::iso::FieldFn(), req, st, &r->meshes, &err);
        }
        if (rc != BBFMM_OK) return iso_fail(h, r, rc, err);
        return BBFMM_OK;
    });
}

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
    static_assert(sizeof(bbfmm::iso::Mesh::closure_stats) == BBFMM_CLOSURE_STATS * sizeof(int64_t), "closure stats");
    return mesh_member(r, i, stats_out, &bbfmm::iso::Mesh::closure_stats);
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
    return mesh_member(r, i, stats_out, &bbfmm::iso::Mesh::isect_stats);
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
    return mesh_member(r, i, stats_out, &bbfmm::iso::Mesh::follow_stats);
}

int bbfmm_isosurface_follow_bricks(const bbfmm_isosurface_result *r, int32_t i, int32_t *dims_out, uint8_t *bricks_out) {
    if (!r || !dims_out || i < 0 || i >= static_cast<int32_t>(r->meshes.size())) return BBFMM_BAD_ARGUMENT;
    const bbfmm::iso::Mesh &m = r->meshes[i];
    std::memcpy(dims_out, m.follow_dims, sizeof(m.follow_dims));
    if (bricks_out && !m.follow_bricks.empty()) std::memcpy(bricks_out, m.follow_bricks.data(), m.follow_bricks.size());
    return BBFMM_OK;
}

int bbfmm_isosurface_follow_times(const bbfmm_isosurface_result *r, int32_t i, double *ms_out) {
    return mesh_member(r, i, ms_out, &bbfmm::iso::Mesh::follow_ms);
}

int bbfmm_isosurface_curvature_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out) {
    return mesh_member(r, i, stats_out, &bbfmm::iso::Mesh::curv_stats);
}

int bbfmm_isosurface_finish_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out) {
    return mesh_member(r, i, stats_out, &bbfmm::iso::Mesh::finish_stats);
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
    return mesh_member(r, i, stats_out, &bbfmm::iso::Mesh::stats);
}

const char *bbfmm_isosurface_error(const bbfmm_isosurface_result *r) { return r ? r->err.c_str() : "null result"; }

void bbfmm_isosurface_destroy(bbfmm_isosurface_result *r) { delete r; }

} // extern "C"
