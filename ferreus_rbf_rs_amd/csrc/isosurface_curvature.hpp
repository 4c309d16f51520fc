// Curvature-weighted cluster points (ferreus_rmt ClusterMethod::CurvatureWeighted, curvature_weighting.rs): the weight of
// one crossed lattice edge as a function that the device kernel and the host entry bbfmm_isosurface_curvature_weight both
// run.  Contract: DESIGN.md "Curvature-weighted clusters"; numpy restatement: tests/isosurface_curvature_restatement.py.
#pragma once
#include "isosurface.hpp"

namespace bbfmm {
namespace iso {

// ---- the reference's tables (ferreus_rmt/src/constants.rs; values checked against tests/golden/rmt_curvature_tables.json)
constexpr double kCurvEps = 1.0e-12;       // EPS, and the bound of Point::unit
constexpr double kCurvMaxCot = 1.0e12;     // MAX_COT_THETA
constexpr double kCurvMaxWeight = 1.0e12;  // MAX_CURVATURE_WEIGHT
constexpr double kCurvPhi[2] = {0.955316618125, 1.230959417341}; // PHI_1, PHI_2
// Rows 0..6 of NEIGHBOUR_EDGE_PLANE_PAIRS (an owned edge has a label below 7): the calculation planes around the edge,
// each the two neighbouring edges of the owner that span it with the edge; rows 1, 3 and 5 have two planes.
constexpr int kCurvPlanes[7] = {3, 2, 3, 2, 3, 2, 3};
constexpr int kCurvPairs[7][3][2] = {{{9, 1}, {12, 4}, {3, 13}}, {{0, 2}, {4, 13}, {-1, -1}}, {{1, 7}, {13, 5}, {4, 10}},
                                     {{9, 4}, {6, 0}, {-1, -1}}, {{0, 5}, {3, 2}, {1, 6}},    {{4, 7}, {2, 6}, {-1, -1}},
                                     {{5, 9}, {7, 3}, {8, 4}}};
// The same rows of NEIGHBOUR_EDGE_PLANE_PHIS as indices into kCurvPhi.
constexpr int kCurvPhis[7][3][2] = {{{1, 0}, {0, 1}, {0, 1}}, {{0, 0}, {0, 0}, {-1, -1}}, {{0, 1}, {1, 0}, {1, 0}},
                                    {{0, 0}, {0, 0}, {-1, -1}}, {{1, 0}, {0, 1}, {0, 1}}, {{0, 0}, {0, 0}, {-1, -1}},
                                    {{0, 1}, {1, 0}, {0, 1}}};

// sin and cos of PHI_1 and PHI_2, computed once on the host (curvature_trig) and passed to the device by value.
struct CurvTrig {
    double sin_phi[2], cos_phi[2];
};
inline CurvTrig curvature_trig() {
    CurvTrig t;
    for (int q = 0; q < 2; ++q) {
        t.sin_phi[q] = std::sin(kCurvPhi[q]);
        t.cos_phi[q] = std::cos(kCurvPhi[q]);
    }
    return t;
}

// Mesh::curv_stats
enum CurvStat : int {
    kCurvEdges = 0,        // crossed edges weighted
    kCurvEdgeFallback = 1, // of those, edges with the fallback weight 1 (curvature_weight_for_edge gave None)
    kCurvClusters = 2,     // clusters placed (the vertices of the mesh before the clip)
    kCurvClusterFallback = 3, // of those, clusters whose weights summed to EPS or less: the candidate of kClusterAverage
    kCurvStats = 4
};

__host__ __device__ inline bool curv_finite(double x) { return x - x == 0.0; }
__host__ __device__ inline double curv_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// Point::unit (geometry/point.rs:103-110): None for a norm of 1e-12 or less
__host__ __device__ inline bool curv_unit(const double *v, double *out) {
#pragma clang fp contract(off)
    const double n = sqrt(curv_dot(v, v));
    if (!(n > kCurvEps)) return false;
    const double s = 1.0 / n;
    for (int a = 0; a < 3; ++a) out[a] = v[a] * s;
    return true;
}

// curvature_weight_for_edge (curvature_weighting.rs:48-234) of the owned edge `label` (< 7) of the sample point `owner`
// (lattice ijk).  get(e): f - isovalue at the owner (e = -1) and at its neighbour along edge e (0..13); a neighbour that
// is missing gives NaN.  World vectors are differences of world(ijk) = lo_world + ijk * spacing of both ends.  false:
// None, the caller then takes the weight 1.
template <class Get>
__host__ __device__ inline bool curvature_weight(const Get &get, const int64_t owner[3], int label, const double lo_world[3],
                                                 const double spacing[3], const CurvTrig &trig, double *weight) {
#pragma clang fp contract(off)
    const double d_o = get(-1), d_a = get(label);
    if (!curv_finite(d_o) || !curv_finite(d_a)) return false;
    double ow[3], oa[3], oa_hat[3];
    for (int a = 0; a < 3; ++a) {
        ow[a] = lo_world[a] + static_cast<double>(owner[a]) * spacing[a];
        const double aw = lo_world[a] + static_cast<double>(owner[a] + kEdgeDeltas[label][a]) * spacing[a];
        oa[a] = aw - ow[a];
    }
    const double oa_len = sqrt(curv_dot(oa, oa));
    if (!(oa_len > kCurvEps)) return false;
    if (!curv_unit(oa, oa_hat)) return false;

    const int planes = kCurvPlanes[label];
    double plane_alpha[3] = {0.0, 0.0, 0.0}, plane_axis[3][3], proj[3] = {0.0, 0.0, 0.0};
    for (int p = 0; p < planes; ++p) {
        double perp[2][3], theta[2], cot[2];
        for (int side = 0; side < 2; ++side) {
            const int nb = kCurvPairs[label][p][side], ph = kCurvPhis[label][p][side];
            const double d_b = get(nb);
            if (!curv_finite(d_b)) return false;
            double ob[3];
            for (int a = 0; a < 3; ++a) {
                const double bw = lo_world[a] + static_cast<double>(owner[a] + kEdgeDeltas[nb][a]) * spacing[a];
                ob[a] = bw - ow[a];
            }
            const double ob_len = sqrt(curv_dot(ob, ob));
            if (!(ob_len > kCurvEps)) return false;
            const double along = curv_dot(ob, oa_hat);
            double across[3];
            for (int a = 0; a < 3; ++a) across[a] = ob[a] - oa_hat[a] * along;
            if (!curv_unit(across, perp[side])) return false;
            // Equation (1)
            const double denominator = (d_o - d_a) * ob_len;
            if (!(fabs(denominator) > kCurvEps)) return false;
            const double ratio = ((d_o - d_b) * oa_len) / denominator;
            const double divisor = ratio - trig.cos_phi[ph];
            const double half_pi = 1.5707963267948966; // FRAC_PI_2
            double th;
            if (fabs(divisor) <= kCurvEps) th = __builtin_signbit(divisor) ? -half_pi : half_pi;
            else th = atan(trig.sin_phi[ph] / divisor);
            const double tan_th = tan(th);
            cot[side] = fabs(tan_th) <= kCurvEps ? __builtin_copysign(kCurvMaxCot, th) : 1.0 / tan_th;
            theta[side] = th;
        }
        plane_alpha[p] = fabs(theta[0]) + fabs(theta[1]); // Equation (2)
        double diff[3];
        for (int a = 0; a < 3; ++a) diff[a] = perp[0][a] - perp[1][a];
        if (!curv_unit(diff, plane_axis[p]))
            for (int a = 0; a < 3; ++a) plane_axis[p][a] = perp[0][a];
        for (int a = 0; a < 3; ++a) proj[a] = proj[a] + (perp[0][a] * cot[0] + perp[1][a] * cot[1]);
    }
    const double scale = planes == 3 ? 2.0 / 3.0 : 1.0;
    double n_raw[3], n_est[3];
    for (int a = 0; a < 3; ++a) n_raw[a] = oa_hat[a] + proj[a] * scale;
    if (!curv_unit(n_raw, n_est)) return false;

    double min_tan = __builtin_inf();
    for (int p = 0; p < planes; ++p) {
        double axis[3];
        if (!curv_unit(plane_axis[p], axis)) return false;
        double sin_gamma = fabs(curv_dot(n_est, axis));
        sin_gamma = sin_gamma < 0.0 ? 0.0 : (sin_gamma > 1.0 ? 1.0 : sin_gamma);
        const double cos_gamma = cos(asin(sin_gamma));
        const double one_minus_cos2 = 1.0 - cos_gamma * cos_gamma;
        const double sin_half = fabs(sin(0.5 * plane_alpha[p]));
        double beta = 0.0;
        if (!(sin_half <= kCurvEps)) {
            const double term = 1.0 / (sin_half * sin_half) - 1.0; // Equation (3)
            if (term < 0.0) return false;
            const double inv_tan2 = one_minus_cos2 * term;
            if (inv_tan2 <= kCurvEps) continue;
            beta = 2.0 * atan(1.0 / sqrt(inv_tan2));
        }
        const double t = fabs(tan(0.5 * beta));
        if (t < min_tan) min_tan = t; // f64::min
    }
    if (!curv_finite(min_tan)) return false;
    // Equation (4)
    if (min_tan <= kCurvEps) {
        *weight = kCurvMaxWeight;
        return true;
    }
    const double w = 1.0 / min_tan;
    *weight = w < kCurvMaxWeight ? w : kCurvMaxWeight;
    return true;
}

} // namespace iso
} // namespace bbfmm
