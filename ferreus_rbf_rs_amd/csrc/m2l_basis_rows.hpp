// The changes of basis of the M2L stages on one row = (right-hand side, cell), one wave per row: node order -> parity basis
// (stage 1's input Mp) and parity basis -> node order (stage 2's output Lp).  The standalone streaming kernels of
// device_m2l.hip and the fused M2M / L2L kernels of device_transfer.hip call the same functions, so both form every value
// by the same expression in the same association.  src and dst may be global memory or LDS.
#pragma once
#include "device.hpp"

namespace bbfmm {

// M_e[j] = M[j] + M[rho j], M_o[j] = M[j] - M[rho j] for the representatives j < n_o, M_e[j] = M[j] on the centre plane
// n_o <= j < n_e of an odd order.  rho j = j + (p - 1 - 2 (j / p1)) p1, p1 = n_e / ceil(p / 2).
__device__ __forceinline__ void m2l_parity_row(const double *src, double *dst, int ne16, int n_e, int n_o, int p, int p1, int lane) {
    for (int j = lane; j < n_e; j += 64) {
        const double v = src[j];
        if (j < n_o) {
            const double w = src[j + (p - 1 - 2 * (j / p1)) * p1];
            dst[j] = v + w;
            dst[ne16 + j] = v - w;
        } else {
            dst[j] = v;
        }
    }
}

// The two-level butterfly of axes 0 and 1: a representative (i0, i1 < ceil(p/2), r < p2) with node m = (i0 p + i1) p2 + r
// reads M at m, rho_x m, rho_y m, rho_x rho_y m and writes ee = (m + x) + (y + xy), eo = (m + x) - (y + xy), oe = (m - x) +
// (y - xy), oo = (m - x) - (y - xy); on a centre plane of an odd order the reflected node is the node itself and the part
// that is odd along that axis does not exist (the even part keeps the value once).  Part ab holds its representatives in
// the order (i0, i1, r).
__device__ __forceinline__ void m2l_parity2_row(const double *src, double *dst, const M2lParityOffsets &off, int p, int p2, int lane) {
    const int h = (p + 1) / 2, f = p / 2;
    for (int e = lane; e < h * h * p2; e += 64) {
        const int i0 = e / (h * p2), i1 = (e - i0 * h * p2) / p2, r = e - (i0 * h + i1) * p2;
        const int m = (i0 * p + i1) * p2 + r;
        const int dx = (p - 1 - 2 * i0) * p * p2, dy = (p - 1 - 2 * i1) * p2; // 0 on the centre planes
        const bool cx = i0 >= f, cy = i1 >= f;
        const double v = src[m], vx = src[m + dx], vy = src[m + dy], vxy = src[m + dx + dy];
        const double e0 = cx ? v : v + vx, e1 = cx ? vy : vy + vxy, o0 = v - vx, o1 = vy - vxy;
        const int je = (i0 * h + i1) * p2 + r, jo = (i0 * f + i1) * p2 + r; // position among the y-even / y-odd representatives
        dst[off.v[0] + je] = cy ? e0 : e0 + e1;
        if (!cy) dst[off.v[1] + jo] = e0 - e1;
        if (!cx) dst[off.v[2] + je] = cy ? o0 : o0 + o1;
        if (!cx && !cy) dst[off.v[3] + jo] = o0 - o1;
    }
}

__device__ __forceinline__ void m2l_parity_row_any(const M2lParityRowArgs &a, const double *src, double *dst, int lane) {
    if (a.axes == 2) m2l_parity2_row(src, dst, a.off, a.p, a.p2, lane);
    else m2l_parity_row(src, dst, a.ne16, a.n_e, a.n_o, a.p, a.p1, lane);
}

// The inverse of m2l_parity_row in two steps, so that a kernel may put other work between the loads and their use:
// representative j < n_e reads L_e[j] and (j < n_o) L_o[j]; emit(m, value) then receives L[j] = L_e[j] + L_o[j] and
// L[rho j] = L_e[j] - L_o[j], on the centre plane L[j] = L_e[j]; every node m < n exactly once over all j.
__device__ __forceinline__ void m2l_unparity_load(const double *src, int ne16, int n_o, int j, double &e, double &o) {
    e = src[j];
    o = j < n_o ? src[ne16 + j] : 0.0;
}

template <class Emit>
__device__ __forceinline__ void m2l_unparity_emit(int n_o, int p, int p1, int j, double e, double o, Emit &&emit) {
    if (j < n_o) {
        emit(j, e + o);
        emit(j + (p - 1 - 2 * (j / p1)) * p1, e - o);
    } else {
        emit(j, e);
    }
}

template <class Emit>
__device__ __forceinline__ void m2l_unparity_row(const double *src, int ne16, int n_e, int n_o, int p, int p1, int lane, Emit &&emit) {
    for (int j = lane; j < n_e; j += 64) {
        double e, o;
        m2l_unparity_load(src, ne16, n_o, j, e, o);
        m2l_unparity_emit(n_o, p, p1, j, e, o, emit);
    }
}

// The inverse of m2l_parity2_row, in the same two steps: representative e = (i0, i1 < ceil(p/2), r < p2) reads ee, eo, oe, oo
// at the columns plan.col() (v[0..3]; a part that is odd along a centre plane does not exist: 0) and emits a = ee + eo, b =
// ee - eo, c = oe + oo, d = oe - oo as L[m] = a + c, L[rho_x m] = a - c, L[rho_y m] = b + d, L[rho_x rho_y m] = b - d; on a
// centre plane the reflected node is the node itself.
__device__ __forceinline__ void m2l_unparity2_load(const double *src, const M2lS2PairsPlan &plan, int p, int p2, int e, double (&v)[4]) {
    const int h = (p + 1) / 2, f = p / 2;
    const int i0 = e / (h * p2), i1 = (e - i0 * h * p2) / p2, r = e - (i0 * h + i1) * p2;
    const bool cx = i0 >= f, cy = i1 >= f;
    const int je = (i0 * h + i1) * p2 + r, jo = (i0 * f + i1) * p2 + r;
    v[0] = src[plan.col(0, je)];
    v[1] = cy ? 0.0 : src[plan.col(1, jo)];
    v[2] = cx ? 0.0 : src[plan.col(2, je)];
    v[3] = cx || cy ? 0.0 : src[plan.col(3, jo)];
}

template <class Emit>
__device__ __forceinline__ void m2l_unparity2_emit(int p, int p2, int e, const double (&v)[4], Emit &&emit) {
    const int h = (p + 1) / 2, f = p / 2;
    const int i0 = e / (h * p2), i1 = (e - i0 * h * p2) / p2, r = e - (i0 * h + i1) * p2;
    const int m = (i0 * p + i1) * p2 + r;
    const int dx = (p - 1 - 2 * i0) * p * p2, dy = (p - 1 - 2 * i1) * p2; // 0 on the centre planes
    const bool cx = i0 >= f, cy = i1 >= f;
    const double ee = v[0], eo = v[1], oe = v[2], oo = v[3];
    const double a = cy ? ee : ee + eo, b = ee - eo, c = cy ? oe : oe + oo, d = oe - oo;
    emit(m, cx ? a : a + c);
    if (!cx) emit(m + dx, a - c);
    if (!cy) emit(m + dy, cx ? b : b + d);
    if (!cx && !cy) emit(m + dx + dy, b - d);
}

template <class Emit>
__device__ __forceinline__ void m2l_unparity2_row(const double *src, const M2lS2PairsPlan &plan, int p, int p2, int lane, Emit &&emit) {
    const int h = (p + 1) / 2;
    for (int e = lane; e < h * h * p2; e += 64) {
        double v[4];
        m2l_unparity2_load(src, plan, p, p2, e, v);
        m2l_unparity2_emit(p, p2, e, v, emit);
    }
}

} // namespace bbfmm
