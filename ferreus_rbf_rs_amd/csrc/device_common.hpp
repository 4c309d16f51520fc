// Hand-written CDNA4 (gfx950) kernels for the BBFMM matvec.  See device.hpp for the
// HBM layout.  Wavefront = 64 everywhere; FP64 throughout (the reference is f64 end
// to end, ferreus_bbfmm/src/traits.rs:20).  One device_*.hip per pass family, kernels and launchers together:
//
//   device_gather.hip      gather/scatter  HBM streaming
//   device_p2m.hip, _l2p   P2M / L2P       Chebyshev anterpolation / interpolation (chebyshev.rs:831-927),
//                                          tensor factors staged in LDS
//   device_transfer.hip    M2M / L2L       sum-factorised 1-D transfers (the reference multiplies by the
//                                          dense Kronecker matrix, bbfmm.rs:742-772,1051-1086; same operator)
//   device_m2l.hip         M2L             two batched small-GEMM stages on v_mfma_f64_4x4x4_f64; operator assembly
//   device_p2p.hip         P2P             direct kernel evaluation, LDS-tiled sources, lanes = target x slice
//   device_wx.hip          M2P / P2L       the same against Chebyshev nodes (pieces shared with P2P: device_direct.hpp)
//   device_selftest.hip    FP64 matrix- and vector-pipe peaks; the element-wise test hooks on kernels.hpp
//
// This header is internal to those files: what more than one of them uses.
#pragma once
#include "device.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <type_traits>

namespace bbfmm {

typedef double v4f64 __attribute__((ext_vector_type(4)));

struct Xyz {
    const double *x, *y, *z;
};
inline Xyz make_xyz(const double *const *p) { return Xyz{p[0], p[1], p[2]}; }

// ------------------------------------------------------------------ Chebyshev helpers
// Per-axis node counts: axes >= d have a single node with S = 1, so 1-D/2-D trees run
// through the same 3-D index arithmetic (node index = (i0*P1 + i1)*P2 + i2).
__device__ inline void axis_sizes(int p, int d, int &P0, int &P1, int &P2) {
    P0 = p;
    P1 = d > 1 ? p : 1;
    P2 = d > 2 ? p : 1;
}

// ------------------------------------------------------------------ Chebyshev factors in registers
// S_j(x) = (2 sum_k T_k(x) T_k(node_j) - 1)/p ; dS_j = (2/p) sum_k T'_k(x) T_k(node_j)
// (chebyshev.rs:47-142), with the constants in the table: q = DevCheb::q, q[j][k] = 2 T_k(node_j) / p and q[j][0] = 1 / p, so
// S_j = sum_k T_k(x) q[j][k] and dS_j = sum_{k >= 1} T'_k(x) q[j][k] -- P multiply-adds per factor and no division (the
// IEEE f64 division is a dozen instructions around a quarter-rate v_rcp_f64; there were P of them per axis and point).
template <int P, bool GRAD>
__device__ inline void cheb_S_reg(double x, const double *__restrict__ q, double (&S)[P], double (&dS)[P]) {
    double T[P], dT[P];
    T[0] = 1.0;
    dT[0] = 0.0;
    if (P > 1) {
        T[1] = x;
        dT[1] = 1.0;
    }
#pragma unroll
    for (int j = 2; j < P; ++j) {
        T[j] = 2.0 * x * T[j - 1] - T[j - 2];
        if (GRAD) dT[j] = 2.0 * T[j - 1] + 2.0 * x * dT[j - 1] - dT[j - 2];
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        double s = q[j * P], ds = 0.0; // T_0 = 1, T'_0 = 0
#pragma unroll
        for (int k = 1; k < P; ++k) {
            const double qk = q[j * P + k];
            s += T[k] * qk;
            if (GRAD) ds += dT[k] * qk;
        }
        S[j] = s;
        dS[j] = GRAD ? ds : 0.0;
    }
}

// ------------------------------------------------------------------ launch helpers
// An integer knob from the environment (callers clamp it and keep it in a function-local static: read once per process).
inline int env_int(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

template <int V> using int_c = std::integral_constant<int, V>;

// Kernel-id dispatch: F is a generic lambda taking std::integral_constant<int, ID>.
template <class F> inline void dispatch_kernel_id(int id, F &&f) {
    switch (id) {
    case kLinear: f(std::integral_constant<int, kLinear>{}); break;
    case kThinPlateSpline: f(std::integral_constant<int, kThinPlateSpline>{}); break;
    case kCubic: f(std::integral_constant<int, kCubic>{}); break;
    case kSpheroidal3: f(std::integral_constant<int, kSpheroidal3>{}); break;
    case kSpheroidal5: f(std::integral_constant<int, kSpheroidal5>{}); break;
    case kSpheroidal7: f(std::integral_constant<int, kSpheroidal7>{}); break;
    case kSpheroidal9: f(std::integral_constant<int, kSpheroidal9>{}); break;
    case kLaplacian: f(std::integral_constant<int, kLaplacian>{}); break;
    case kOneOverR2: f(std::integral_constant<int, kOneOverR2>{}); break;
    case kOneOverR4: f(std::integral_constant<int, kOneOverR4>{}); break;
    case kGaussianExt: f(std::integral_constant<int, kGaussianExt>{}); break;
    case kMultiquadricExt: f(std::integral_constant<int, kMultiquadricExt>{}); break;
    default: break;
    }
}

// Order dispatch, like dispatch_kernel_id: f(std::integral_constant<int, P>{}) for the P in LO..HI that equals p;
// false (and no call) for any other p.
template <int LO, int HI, class F> inline bool dispatch_order(int p, F &&f) {
    if constexpr (LO <= HI) {
        if (p != LO) return dispatch_order<LO + 1, HI>(p, f);
        f(std::integral_constant<int, LO>{});
        return true;
    }
    return false;
}

inline int device_cu_count() { // of the current device (every entry point binds its thread to the handle's device)
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev >= 0 && dev < 64) {
        const int c = cache[dev].load(std::memory_order_relaxed);
        if (c > 0) return c;
    }
    int n_cu = 256;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0) n_cu = 256;
    if (dev >= 0 && dev < 64) cache[dev].store(n_cu, std::memory_order_relaxed);
    return n_cu;
}

// Dynamic LDS above the 64 KB default needs the function attribute, per device (3-D orders 14-16 of the general
// M2M / L2L kernels): set once per (kernel, device) -- `done` is that kernel's flag word, set from
// whichever thread launches there first (handles are bound to their device and may be used from any host thread) --
// and a failure is returned to the caller instead of surfacing later as a generic launch error.
inline hipError_t allow_large_dynamic_lds(const void *fn, size_t bytes, std::atomic<uint64_t> *done) {
    if (bytes <= 64 * 1024) return hipSuccess;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const bool cached = dev >= 0 && dev < 256;
    if (cached && ((done[dev >> 6].load(std::memory_order_acquire) >> (dev & 63)) & 1)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess && cached) done[dev >> 6].fetch_or(uint64_t(1) << (dev & 63), std::memory_order_release);
    return e;
}

} // namespace bbfmm
