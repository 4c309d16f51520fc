// The pair predicate of the self-intersection detector: is_true_self_intersection of ferreus_rmt
// (mesh_intersections.rs:125-159) with everything it calls -- tri_tri_intersect (moller.rs:81-147), is_degenerate,
// max_plane_distance_to, segment_pierces_interior, point_in_interior (geometry/triangle.rs:108-183), unit, close_to, lerp
// (geometry/point.rs:103-126) -- as one __host__ __device__ function, so that the host export the tests call and the
// device kernel run the same code.  The reference's constants and its order of tests are kept: tolerance 1e-8, Moeller
// EPSILON 1e-6 (|n1 x n2|^2 <= EPSILON^2 is "parallel", an overlap must exceed EPSILON), unit() gives nothing at a norm
// <= 1e-12.  Every sum is written in the reference's order, without fused multiply-add, with IEEE division and square
// root: host and device take the same branch on the same bits.
//
// The Moeller parallel test uses unnormalised normals, so it depends on the scale of the mesh: the smaller the triangles,
// the more pairs it calls parallel (at edge lengths around 0.1 about 4 in 10 box-overlapping pairs of a noisy surface,
// on a smooth one nearly all).  That is the reference's behaviour and it is reproduced, not repaired.
//
// The predicate is not symmetric in its last bits (shared_vertex_extra_crossing returns at the first coincident (i, j)):
// `a` is the facet with the lower index.  numpy restatement: tests/isosurface_intersect_restatement.py.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bbfmm {
namespace iso {

constexpr double kIsectTolerance = 1.0e-8; // DEFAULT_INTERSECTION_TOLERANCE
constexpr double kMollerEpsilon = 1.0e-6;  // moller.rs EPSILON
constexpr double kUnitMinNorm = 1.0e-12;   // Point::unit

// The test that decided a pair (bbfmm_isosurface_triangle_pair's stage_out).
enum PairStage : int {
    kPairDegenerate = 0,    // a or b has twice its area <= tolerance^2: false
    kPairSharedTwo = 1,     // two or three shared vertex ids: false
    kPairMoller = 2,        // tri_tri_intersect said no: false
    kPairSharedCrossing = 3, // one shared id: shared_vertex_extra_crossing decides
    kPairGeometricShared = 4, // no shared id, coincident vertices: two or more false, one: the crossing test decides
    kPairNearCoplanar = 5,  // one triangle within tolerance of the other's plane: false
    kPairTrue = 6,          // a true self-intersection
    kPairStages = 7
};

struct Vec3 {
    double x[3];
};

__host__ __device__ inline double isect_abs(double v) { return v < 0 ? -v : v; }
// f64::max / f64::min: the other operand where one is NaN
__host__ __device__ inline double isect_max(double a, double b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }
__host__ __device__ inline double isect_min(double a, double b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }

__host__ __device__ inline Vec3 v_sub(const Vec3 &a, const Vec3 &b) {
#pragma clang fp contract(off)
    return Vec3{{a.x[0] - b.x[0], a.x[1] - b.x[1], a.x[2] - b.x[2]}};
}
__host__ __device__ inline double v_dot(const Vec3 &a, const Vec3 &b) {
#pragma clang fp contract(off)
    return a.x[0] * b.x[0] + a.x[1] * b.x[1] + a.x[2] * b.x[2];
}
__host__ __device__ inline Vec3 v_cross(const Vec3 &a, const Vec3 &b) {
#pragma clang fp contract(off)
    return Vec3{{a.x[1] * b.x[2] - a.x[2] * b.x[1], a.x[2] * b.x[0] - a.x[0] * b.x[2], a.x[0] * b.x[1] - a.x[1] * b.x[0]}};
}
__host__ __device__ inline double v_norm(const Vec3 &a) { return __builtin_sqrt(v_dot(a, a)); }
// Point::unit; false: too close to zero
__host__ __device__ inline bool v_unit(const Vec3 &a, Vec3 *u) {
#pragma clang fp contract(off)
    const double n = v_norm(a);
    if (n <= kUnitMinNorm) return false;
    const double s = 1.0 / n;
    *u = Vec3{{a.x[0] * s, a.x[1] * s, a.x[2] * s}};
    return true;
}
__host__ __device__ inline bool v_close(const Vec3 &a, const Vec3 &b, double tol) { return v_norm(v_sub(a, b)) <= tol; }

struct Tri3 {
    Vec3 p[3];
};

__host__ __device__ inline Vec3 tri_normal(const Tri3 &t) { return v_cross(v_sub(t.p[1], t.p[0]), v_sub(t.p[2], t.p[0])); }

// isect (moller.rs:33-37)
__host__ __device__ inline void moller_isect(double vv0, double vv1, double vv2, double d0, double d1, double d2, double *i0, double *i1) {
#pragma clang fp contract(off)
    *i0 = vv0 + (vv1 - vv0) * d0 / (d0 - d1);
    *i1 = vv0 + (vv2 - vv0) * d0 / (d0 - d2);
}

// compute_intervals (moller.rs:39-62)
__host__ __device__ inline bool moller_intervals(double vv0, double vv1, double vv2, double d0, double d1, double d2, double d0d1,
                                                 double d0d2, double *i0, double *i1) {
#pragma clang fp contract(off)
    if (d0d1 > 0.0) moller_isect(vv2, vv0, vv1, d2, d0, d1, i0, i1);
    else if (d0d2 > 0.0) moller_isect(vv1, vv0, vv2, d1, d0, d2, i0, i1);
    else if (d1 * d2 > 0.0 || d0 != 0.0) moller_isect(vv0, vv1, vv2, d0, d1, d2, i0, i1);
    else if (d1 != 0.0) moller_isect(vv1, vv0, vv2, d1, d0, d2, i0, i1);
    else if (d2 != 0.0) moller_isect(vv2, vv0, vv1, d2, d0, d1, i0, i1);
    else return false;
    return true;
}

// tri_tri_intersect (moller.rs:81-147): proper intersections only, no single-point contact, no coplanar overlap
__host__ __device__ inline bool moller_tri_tri(const Tri3 &t1, const Tri3 &t2) {
#pragma clang fp contract(off)
    const Vec3 &v0 = t1.p[0], &v1 = t1.p[1], &v2 = t1.p[2], &u0 = t2.p[0], &u1 = t2.p[1], &u2 = t2.p[2];
    const Vec3 n1 = v_cross(v_sub(v1, v0), v_sub(v2, v0));
    const double d1 = -v_dot(n1, v0);
    const double du0 = v_dot(n1, u0) + d1, du1 = v_dot(n1, u1) + d1, du2 = v_dot(n1, u2) + d1;
    const double du0du1 = du0 * du1, du0du2 = du0 * du2;
    if (du0du1 > 0.0 && du0du2 > 0.0) return false;
    const Vec3 n2 = v_cross(v_sub(u1, u0), v_sub(u2, u0));
    const double d2 = -v_dot(n2, u0);
    const double dv0 = v_dot(n2, v0) + d2, dv1 = v_dot(n2, v1) + d2, dv2 = v_dot(n2, v2) + d2;
    const double dv0dv1 = dv0 * dv1, dv0dv2 = dv0 * dv2;
    if (dv0dv1 > 0.0 && dv0dv2 > 0.0) return false;
    const Vec3 dir = v_cross(n1, n2);
    if (v_dot(dir, dir) <= kMollerEpsilon * kMollerEpsilon) return false;
    int index = 0; // dominant_axis
    double mx = isect_abs(dir.x[0]);
    if (isect_abs(dir.x[1]) > mx) {
        index = 1;
        mx = isect_abs(dir.x[1]);
    }
    if (isect_abs(dir.x[2]) > mx) index = 2;
    double a0, a1, b0, b1;
    if (!moller_intervals(v0.x[index], v1.x[index], v2.x[index], dv0, dv1, dv2, dv0dv1, dv0dv2, &a0, &a1)) return false;
    if (!moller_intervals(u0.x[index], u1.x[index], u2.x[index], du0, du1, du2, du0du1, du0du2, &b0, &b1)) return false;
    if (a0 > a1) { const double s = a0; a0 = a1; a1 = s; }
    if (b0 > b1) { const double s = b0; b0 = b1; b1 = s; }
    const double start = isect_max(a0, b0), end = isect_min(a1, b1);
    return end - start > kMollerEpsilon;
}

// point_in_interior (geometry/triangle.rs:147-161)
__host__ __device__ inline bool tri_point_in_interior(const Tri3 &t, const Vec3 &q, double tol) {
#pragma clang fp contract(off)
    Vec3 n;
    if (!v_unit(tri_normal(t), &n)) return false;
    if (isect_abs(v_dot(v_sub(q, t.p[0]), n)) > tol) return false;
    const double c0 = v_dot(v_cross(v_sub(t.p[1], t.p[0]), v_sub(q, t.p[0])), n);
    const double c1 = v_dot(v_cross(v_sub(t.p[2], t.p[1]), v_sub(q, t.p[1])), n);
    const double c2 = v_dot(v_cross(v_sub(t.p[0], t.p[2]), v_sub(q, t.p[2])), n);
    const double at = tol * tol;
    return (c0 > at && c1 > at && c2 > at) || (c0 < -at && c1 < -at && c2 < -at);
}

// segment_pierces_interior (geometry/triangle.rs:167-183)
__host__ __device__ inline bool tri_segment_pierces(const Tri3 &t, const Vec3 &p0, const Vec3 &p1, double tol) {
#pragma clang fp contract(off)
    Vec3 n;
    if (!v_unit(tri_normal(t), &n)) return false;
    const double d0 = v_dot(v_sub(p0, t.p[0]), n), d1 = v_dot(v_sub(p1, t.p[0]), n);
    if (isect_abs(d0) <= tol || isect_abs(d1) <= tol || d0 * d1 >= 0.0) return false;
    const double s = d0 / (d0 - d1);
    if (s <= tol || s >= 1.0 - tol) return false;
    const Vec3 d = v_sub(p1, p0); // lerp: p0 + (p1 - p0) * s
    const Vec3 q{{p0.x[0] + d.x[0] * s, p0.x[1] + d.x[1] * s, p0.x[2] + d.x[2] * s}};
    return tri_point_in_interior(t, q, tol);
}

// max_plane_distance_to (geometry/triangle.rs:135-141): a degenerate t is infinitely far
__host__ __device__ inline double tri_max_plane_distance(const Tri3 &t, const Tri3 &other) {
#pragma clang fp contract(off)
    Vec3 n;
    if (!v_unit(tri_normal(t), &n)) return __builtin_inf();
    double m = 0.0;
    for (int k = 0; k < 3; ++k) m = isect_max(m, isect_abs(v_dot(v_sub(other.p[k], t.p[0]), n)));
    return m;
}

// shared_vertex_extra_crossing (mesh_intersections.rs:103-118): decided at the first coincident (i, j); the edge
// opposite vertex i is edges()[(i + 1) % 3] = (p[(i + 1) % 3], p[(i + 2) % 3])
__host__ __device__ inline bool pair_extra_crossing(const Tri3 &a, const Tri3 &b, double tol) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            if (!v_close(a.p[i], b.p[j], tol)) continue;
            return tri_segment_pierces(b, a.p[(i + 1) % 3], a.p[(i + 2) % 3], tol) ||
                   tri_segment_pierces(a, b.p[(j + 1) % 3], b.p[(j + 2) % 3], tol);
        }
    return false;
}

// is_true_self_intersection (mesh_intersections.rs:125-159); a: the facet with the lower index.  *stage: PairStage.
__host__ __device__ inline bool triangle_pair(const Tri3 &a, const int64_t ia[3], const Tri3 &b, const int64_t ib[3], int *stage) {
#pragma clang fp contract(off)
    const double tol = kIsectTolerance;
    *stage = kPairDegenerate;
    if (v_norm(tri_normal(a)) <= tol * tol || v_norm(tri_normal(b)) <= tol * tol) return false;
    int shared = 0; // shared_vertex_count: the ids of a that b holds
    for (int i = 0; i < 3; ++i)
        if (ia[i] == ib[0] || ia[i] == ib[1] || ia[i] == ib[2]) ++shared;
    *stage = kPairSharedTwo;
    if (shared >= 2) return false;
    *stage = kPairMoller;
    if (!moller_tri_tri(a, b)) return false;
    *stage = kPairSharedCrossing;
    if (shared == 1) return pair_extra_crossing(a, b, tol);
    int geometric = 0; // geometric_shared_vertex_count (mesh_intersections.rs:65-78)
    bool used[3] = {false, false, false};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (!used[j] && v_close(a.p[i], b.p[j], tol)) {
                used[j] = true;
                ++geometric;
                break;
            }
    *stage = kPairGeometricShared;
    if (geometric >= 2) return false;
    if (geometric == 1) return pair_extra_crossing(a, b, tol);
    *stage = kPairNearCoplanar;
    if (isect_min(tri_max_plane_distance(a, b), tri_max_plane_distance(b, a)) <= tol) return false; // near_coplanar
    *stage = kPairTrue;
    return true;
}

} // namespace iso
} // namespace bbfmm
